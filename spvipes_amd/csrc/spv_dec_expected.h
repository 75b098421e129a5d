// Denoised-expression read-out: the mean of the decoder's NB mixture, its two parts or its mixing weight, over a selected
// list of genes, as ONE row-major fp32 array (spv_dec_expected; get_normalized_expression of the user API).
//
// Reference semantics (file:line into /root/reference/src/spVIPES): nn/networks.py:314-325 and module/spVIPESmodule.py:751-759 --
//   rate_k = exp(library) * softmax_G(BN_G(z_k W_k^T)), k in {private, shared};  pi = sigmoid(mixing logits) weights component 1
//   (the private rate);  mixture mean = pi * rate_private + (1 - pi) * rate_shared.
//
// How the work is laid out on the chip
//   * A workgroup owns 32 cells (one MFMA column tile) and stages their rows of the logits operand Am ([32][K <= 320] bf16, hi and
//     lo planes in fp32 mode) in LDS once; its four waves then walk 32-gene tiles of the SELECTION.  Lane r of a wave holds the
//     id of selected gene tile0 + r and reads that gene's rows of Wps and Wm itself (a gather of 16-byte pieces from L2): the
//     gene-side MFMA fragments are "row per lane", so a gene list costs nothing but the index load.
//   * y_private / y_shared are evaluated exactly as dec_lse_kernel / dec_materialize_kernel evaluate them (ps_eval: the same split-bf16
//     MFMAs in the same K order; genes on MFMA rows, cells on columns), the logits as the logits GEMM accumulates them (K steps of
//     16 in order, hi * lo, lo * hi, hi * hi per step, fp32 accumulators), so an element's value depends on its own gene and cell only.
//   * The accumulator layout is lane = cell, registers = genes; a store from it would put every lane on its own output row.  Each wave
//     therefore turns its finished 32 x 32 tile through a private LDS tile and stores it with lane = gene: 32 consecutive lanes write
//     128 consecutive bytes of one cell's row.
#pragma once
#include "spv_decoder.h"

namespace spv {

constexpr int DX_CELLS = 32;     // cells per workgroup
constexpr int DX_KMAX = 320;     // widest logits operand
constexpr int DX_APITCH = 328;   // LDS row pitch of the staged Am rows in bf16 (164 dwords = 4 mod 32: conflict-free 16-byte row reads)
constexpr int DX_TPITCH = 36;    // row pitch of a wave's transpose tile in floats
constexpr int DX_PLANE = DX_CELLS * DX_APITCH;   // one staged plane of Am (the lo plane follows the hi plane in fp32 mode)

struct DecExpArgs {
  const bf16_t *Am_hi, *Am_lo, *Wm_hi, *Wm_lo;   // [Bp][K], [Gp][K]
  int K;
  const int* genes; int n_genes; int what;
  float* out; long ld_out;
  float alpha; int accumulate;
};

// wave-local hand-over through LDS (the four waves of a workgroup never exchange data after the staging barrier)
__device__ __forceinline__ void dx_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// what: 0 mixture mean, 1 private part pi * rate_p, 2 shared part (1 - pi) * rate_s, 3 pi.  pi and 1 - pi are both formed from
// exp(-|logit|), so neither loses digits next to 1; the mean is the rounded sum of the two rounded parts (no contraction), which
// makes "part 1 + part 2 == mean" hold to the last bit of one fp32 addition.
__device__ __forceinline__ float dx_value(int what, float rp, float rs, float logit) {
#pragma clang fp contract(off)
  const float e = __expf(-fabsf(logit)), inv = fast_rcp(1.0f + e), small = e * inv;
  const float pi = (logit >= 0.f) ? inv : small, qi = (logit >= 0.f) ? small : inv;
  const float vp = pi * rp, vs = qi * rs;
  return what == 0 ? vp + vs : what == 1 ? vp : what == 2 ? vs : pi;
}

// one K step of 16 of the logits contraction: A = the lane's gene row of Wm (global), B = the lane's cell row of Am (LDS)
template <int NSPLIT>
__device__ __forceinline__ f16v dx_logit_step(const bf16_t* wm_hi, const bf16_t* wm_lo, long wrow, const bf16_t* arow, int k, f16v acc) {
  const s8v wh = *reinterpret_cast<const s8v*>(wm_hi + wrow + k);
  const s8v ah = *reinterpret_cast<const s8v*>(arow + k);
  s8v wl = wh, al = ah;
  if constexpr (NSPLIT == 3) {
    wl = *reinterpret_cast<const s8v*>(wm_lo + wrow + k);
    al = *reinterpret_cast<const s8v*>(arow + DX_PLANE + k);
  }
  return mfma32_split<NSPLIT>(wh, wl, ah, al, acc);
}

// The decode front-end that dec_expected_kernel and dec_sample_kernel (spv_dec_sample.h) share: everything up to a tile's yp / ys / logit
// accumulators.  Pointers are parameters, so a kernel may hand in laundered copies (nbs_in_vgpr).

// stage the workgroup's 32 cells' rows of Am (s_am: one plane, two in fp32 mode); the caller's __syncthreads() publishes them
template <int NSPLIT>
__device__ __forceinline__ void dx_stage_am(bf16_t* s_am, const bf16_t* Am_hi, const bf16_t* Am_lo, int K, int cell0, int tid) {
  const int kch = K >> 3;   // 16-byte pieces per row
  for (int i = tid; i < DX_CELLS * kch; i += 256) {
    const int row = i / kch, ch = i - row * kch;
    const long src = (long)(cell0 + row) * K + 8 * ch;
    *reinterpret_cast<u4v*>(s_am + row * DX_APITCH + 8 * ch) = *reinterpret_cast<const u4v*>(Am_hi + src);
    if constexpr (NSPLIT == 3) *reinterpret_cast<u4v*>(s_am + DX_PLANE + row * DX_APITCH + 8 * ch) = *reinterpret_cast<const u4v*>(Am_lo + src);
  }
}

// lane r's gene of the tile at sel0: a column beyond the selection re-reads the last one (never stored); ids are clamped into [0, G)
__device__ __forceinline__ int dx_tile_gene(const int* genes, int n_genes, int sel0, int r, int G) {
  const int si = min(sel0 + r, n_genes - 1);
  const int g = genes ? genes[si] : si;
  return min(max(g, 0), G - 1);
}

// gene g's 32 x 32 tile against the staged cells: yp / ys by ps_eval, acc = the mixing logits (arow: the lane's staged row of Am)
template <int NSPLIT, int KW>
__device__ __forceinline__ void dx_decode_tile(const bf16_t* wps_hi, const bf16_t* wps_lo, const bf16_t* wm_hi, const bf16_t* wm_lo, int K, int g, int h,
                                               const bf16_t* arow, const PsFragsK<KW>& cf, f16v& yp, f16v& ys, f16v& acc) {
  // ---- rate heads: the gene's rows of the folded regressor image ------------------------------------------------------
  PsWK<KW> w;
  {
    const long off = (long)g * DEC_KPS_W<KW> + 8 * h;
#pragma unroll
    for (int s = 0; s < 3 * KW; ++s) {
      w.hi[s] = *reinterpret_cast<const s8v*>(wps_hi + off + 16 * s);
      w.lo[s] = *reinterpret_cast<const s8v*>(wps_lo + off + 16 * s);
    }
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) { yp[q] = 0.f; ys[q] = 0.f; acc[q] = 0.f; }
  ps_eval(w, cf, yp, ys);
  // ---- mixing logits of the tile: K steps of 16 in order ---------------------------------------------------------------
  const long wrow = (long)g * K + 8 * h;
  if (K == DX_KMAX) {   // the width dec_ops packs: fully unrolled, so the gathers of the gene's row are all issued ahead of the MFMA chain
#pragma unroll
    for (int k = 0; k < DX_KMAX; k += 16) acc = dx_logit_step<NSPLIT>(wm_hi, wm_lo, wrow, arow, k, acc);
  } else {
    for (int k0 = 0; k0 < K; k0 += 32) {   // (K % 32 == 0)
      acc = dx_logit_step<NSPLIT>(wm_hi, wm_lo, wrow, arow, k0, acc);
      acc = dx_logit_step<NSPLIT>(wm_hi, wm_lo, wrow, arow, k0 + 16, acc);
    }
  }
}

template <int NSPLIT, int KW>
__global__ __launch_bounds__(256) void dec_expected_kernel(DecParams p, DecExpArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t s_am[(NSPLIT == 3 ? 2 : 1) * DX_PLANE];
  __shared__ __attribute__((aligned(16))) float s_t[4][32 * DX_TPITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, r = lane & 31;
  const int cell0 = blockIdx.x * DX_CELLS;   // (cell0 + 32 <= Bp: the grid has Bp / 32 columns)
  dx_stage_am<NSPLIT>(s_am, a.Am_hi, a.Am_lo, a.K, cell0, tid);
  PsFragsK<KW> cf;
  load_ps_cell_frags(p, cell0, lane, cf);
  const float ap = p.a_p[cell0 + r], as = p.a_s[cell0 + r];
  __syncthreads();
  const int ntiles = (a.n_genes + 31) >> 5;
  float* const tile = s_t[wave];
  const bf16_t* const arow = s_am + r * DX_APITCH + 8 * h;
  for (int t = blockIdx.y * 4 + wave; t < ntiles; t += gridDim.y * 4) {
    const int sel0 = t * 32;
    f16v yp, ys, acc;
    dx_decode_tile<NSPLIT, KW>(p.Wps_hi, p.Wps_lo, a.Wm_hi, a.Wm_lo, a.K, dx_tile_gene(a.genes, a.n_genes, sel0, r, p.G), h, arow, cf, yp, ys, acc);
    // ---- values -> the wave's LDS tile [cell r][gene crow(q, h)] ---------------------------------------------------------
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      f4v v;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int q = 4 * qq + j;
        v[j] = dx_value(a.what, __expf(yp[q] + ap), __expf(ys[q] + as), acc[q]);
      }
      *reinterpret_cast<f4v*>(tile + r * DX_TPITCH + 8 * qq + 4 * h) = v;
    }
    dx_wave_sync();
    // ---- store with lane = gene: rows 2 i + h, 32 consecutive floats each -----------------------------------------------
    const int col = sel0 + r;
    if (col < a.n_genes) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int c = 2 * i + h, cell = cell0 + c;
        if (cell < p.B) {
          float* const o = a.out + (long)cell * a.ld_out + col;
          float v = a.alpha * tile[c * DX_TPITCH + r];
          if (a.accumulate) v += *o;
          *o = v;
        }
      }
    }
    dx_wave_sync();   // the tile is rewritten by the next iteration
  }
}

}  // namespace spv
