// Posterior-predictive counts: draws from the decoder's NB mixture (spv_dec_sample; posterior_predictive_sample of the user API),
// and the same sampler over given parameter arrays (spv_nbmix_sample).
//
// Reference semantics (file:line into the reference's src/spVIPES): module/spVIPESmodule.py:751-759 --
//   NegativeBinomialMixture(mu1 = rate_private, mu2 = rate_shared, theta1 = exp(px_r), mixture_logits = px_mixing), no theta2: both
//   components share theta.  scvi-tools draws it per (cell, gene) as
//     c ~ Bernoulli(pi), pi = sigmoid(mixing logit) (component 1 = the private rate);   mu = c ? rate_private : rate_shared;
//     lam = Gamma(shape = theta, scale = mu / theta), clamped at 1e8;                   x ~ Poisson(lam).
//
// Random stream.  Uniforms are 23-bit fractions (k + 1/2) 2^-23 of Philox 4x32-10 words; the block that holds them is addressed by
//   counter = (gene id, cell id, sample index, block number), key = the caller's 64-bit key,
// so a draw depends on its own gene, cell, sample and key only -- not on the grid, the tile, the position of the gene in a selection
// or on what the other lanes do.  Block 0 holds the one-shot uniforms (component, the shape < 1 boost, the inversion uniform or the
// normal of the large-lam regime); attempt j of the Gamma rejection loop reads block NBS_BLK_GAMMA + j, attempt j of the Poisson
// rejection loop block NBS_BLK_PTRS + j: a retry takes the next block number.
//
// Regimes (DESIGN.md section 13 has the derivations):
//   Gamma    shape >= 1  Marsaglia-Tsang (2000);  shape < 1  Gamma(shape + 1) * U^(1 / shape) (may underflow to 0: correct)
//   Poisson  lam < 10  sequential inversion from one uniform;  10 <= lam <= 2^20  Hoermann's PTRS (1993) with the log-pmf in
//            Loader's saddle-point form (no cancellation between k log lam, lam and lgamma(k + 1));  lam > 2^20  rounded normal
// Every loop has a fixed trip cap and a deterministic fall-back value (reached with probability < 2^-40 per element), no loop
// waits on another lane, and the loops hold no MFMA, cross-lane operation or barrier.
#pragma once
#include "spv_dec_expected.h"

namespace spv {

constexpr int NBS_GAMMA_CAP = 12;     // Marsaglia-Tsang rejects with probability < 0.05 for every shape >= 1:  0.05^12  = 2^-51.9
constexpr int NBS_PTRS_CAP = 24;      // PTRS rejects with probability <= 1 - 1 / 1.329 = 0.2476 at lam >= 10:   0.2476^24 = 2^-48.3
constexpr int NBS_INV_CAP = 64;       // P(Poisson(10) >= 64) = 2^-93
constexpr unsigned NBS_BLK_GAMMA = 1, NBS_BLK_PTRS = NBS_BLK_GAMMA + NBS_GAMMA_CAP;
constexpr float NBS_LAM_INV = 10.0f;          // below: inversion
constexpr float NBS_LAM_NORMAL = 1048576.0f;  // above: rounded normal (skewness 2^-10; a 23-bit uniform no longer resolves PTRS's hat)
constexpr float NBS_LAM_MAX = 1.0e8f;         // scvi-tools' clamp of the Gamma draw

struct NbStream { unsigned key[2]; unsigned gene, cell, sample; };

__device__ __forceinline__ void nbs_block(const NbStream& st, unsigned block, unsigned (&w)[4]) {
  w[0] = st.gene; w[1] = st.cell; w[2] = st.sample; w[3] = block;
  philox4x32_10(w, st.key);
}
// (k + 1/2) 2^-23, k < 2^23: exact in fp32, strictly inside (0, 1)
__device__ __forceinline__ float nbs_u23(unsigned w) { return ((float)(w >> 9) + 0.5f) * (1.0f / 8388608.0f); }
// one standard normal from two uniforms (Box-Muller, the cosine branch; |z| <= 5.65)
__device__ __forceinline__ float nbs_normal(float u1, float u2) { return sqrtf(-2.0f * __logf(u1)) * __builtin_amdgcn_cosf(u2); }

// log of the Poisson pmf at a whole number k >= 0, lam >= 10.  k < 10: k log lam - lam - log k! with the factorial as an exact
// product.  Else Loader's form  -1/2 log(2 pi k) - stirlerr(k) - bd0(k, lam),  bd0 = k log(k / lam) + lam - k  evaluated by its
// series in v = (k - lam) / (k + lam) next to the mode, where the three terms of the textbook form cancel (at lam = 2^20 they are
// 1.4e7 each and an fp32 ulp of them is 1: the acceptance test would be noise).
__device__ __forceinline__ float nbs_pois_logpmf(float k, float lam, float loglam) {
  if (k < 10.0f) {
    float f = 1.0f;
#pragma unroll
    for (int i = 2; i < 10; ++i) f *= ((float)i <= k) ? (float)i : 1.0f;
    return k * loglam - lam - __logf(f);
  }
  const float ik = fast_rcp(k), ik2 = ik * ik;
  const float stirl = ik * (0.08333333333333333f - ik2 * (0.002777777777777778f - ik2 * 0.0007936507936507937f));
  const float dlt = k - lam, sum = k + lam;
  float bd0;
  if (fabsf(dlt) < 0.1f * sum) {
    const float v = dlt / sum, v2 = v * v;   // v2 <= 0.01: the term after v2^6 / 13 is below 1e-15 of the first
    const float ser = v2 * (0.3333333333333333f + v2 * (0.2f + v2 * (0.14285714285714285f + v2 * (0.1111111111111111f + v2 * (0.09090909090909091f + v2 * 0.07692307692307693f)))));
    bd0 = dlt * v + 2.0f * k * v * ser;
  } else {
    bd0 = k * __logf(k / lam) + lam - k;
  }
  return -0.5f * __logf(6.283185307179586f * k) - stirl - bd0;
}

// Poisson(lam), 0 < lam <= NBS_LAM_MAX.  b0: the element's block 0 (words 2 and 3 are this stage's).
__device__ __forceinline__ int nbs_poisson(const NbStream& st, const unsigned (&b0)[4], float lam) {
  if (lam < NBS_LAM_INV) {
    // sequential inversion: the first k with u <= P(X <= k).  The partial sums stop growing once a term is below 2^-30 (past the mode);
    // a u in the last ulps below 1 that they never reach ends there (probability < 2^-22 of an index whose pmf is < 2^-30).
    const float u = nbs_u23(b0[2]);
    float p = __expf(-lam), s = p;
    int k = 0;
    while (u > s && k < NBS_INV_CAP) {
      ++k;
      p *= lam * fast_rcp((float)k);
      s += p;
      if (p < 9.3e-10f && (float)k > lam) break;
    }
    return k;
  }
  if (lam > NBS_LAM_NORMAL) {
    const float z = nbs_normal(nbs_u23(b0[2]), nbs_u23(b0[3]));
    return (int)fmaxf(floorf(lam + sqrtf(lam) * z + 0.5f), 0.0f);
  }
  // PTRS (W. Hoermann, "The transformed rejection method for generating Poisson random variables", 1993), constants as published.
  // lam = L + f with L whole: the candidate is L + floor(hat(U) + f + 0.43), so the floor acts on a number of size ~sqrt(lam).
  const float slam = sqrtf(lam), loglam = __logf(lam);
  const float b = 0.931f + 2.53f * slam, a = -0.059f + 0.02483f * b;
  const float invalpha = 1.1239f + 1.1328f / (b - 3.4f), vr = 0.9277f - 3.6224f / (b - 2.0f);
  const float L = floorf(lam), f = lam - L;
  float res = floorf(lam + 0.5f);   // the cap's fall-back
  for (int j = 0; j < NBS_PTRS_CAP; ++j) {
    unsigned w[4];
    nbs_block(st, NBS_BLK_PTRS + j, w);
    const float U = nbs_u23(w[0]) - 0.5f, V = nbs_u23(w[1]);
    const float us = 0.5f - fabsf(U);
    const float k = L + floorf((2.0f * a / us + b) * U + f + 0.43f);
    if (us >= 0.07f && V <= vr) { res = k; break; }
    if (k < 0.0f || k > 2.0e9f || (us < 0.013f && V > us)) continue;
    if (__logf(V * invalpha / (a / (us * us) + b)) <= nbs_pois_logpmf(k, lam, loglam)) { res = k; break; }
  }
  return (int)res;
}

// Gamma(shape = theta, scale = 1).  b0: the element's block 0 (word 1 is this stage's).
__device__ __forceinline__ float nbs_gamma(const NbStream& st, const unsigned (&b0)[4], float theta) {
  const bool boost = theta < 1.0f;
  const float shape = boost ? theta + 1.0f : theta;
  const float d = shape - 0.3333333333333333f, c = rsqrtf(9.0f * d);
  float g = d;   // the cap's fall-back: v = 1
  for (int j = 0; j < NBS_GAMMA_CAP; ++j) {
    unsigned w[4];
    nbs_block(st, NBS_BLK_GAMMA + j, w);
    const float x = nbs_normal(nbs_u23(w[0]), nbs_u23(w[1])), u = nbs_u23(w[2]);
    const float t = 1.0f + c * x, v = t * t * t, x2 = x * x;
    if (t > 0.0f && (u < 1.0f - 0.0331f * x2 * x2 || __logf(u) < 0.5f * x2 + d * (1.0f - v + __logf(v)))) { g = d * v; break; }
  }
  if (boost) g *= __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(nbs_u23(b0[1])) / theta);
  return g;
}

// One draw of the NB mixture.  pi is formed as dx_value forms it.  A selected rate or a theta that is NaN, zero or negative gives 0,
// and so does a Gamma draw that underflowed to 0; every path ends after a bounded number of steps whatever the inputs are.
__device__ __forceinline__ int nbmix_draw(const NbStream& st, float rate_p, float rate_s, float theta, float logit) {
  unsigned b0[4];
  nbs_block(st, 0, b0);
  const float e = __expf(-fabsf(logit)), inv = fast_rcp(1.0f + e), small = e * inv;
  const float pi = (logit >= 0.f) ? inv : small;
  const float mu = (nbs_u23(b0[0]) < pi) ? rate_p : rate_s;
  if (!(mu > 0.0f) || !(theta > 0.0f)) return 0;   // (NaN compares false)
  const float raw = nbs_gamma(st, b0, theta) * (mu / theta);
  if (!(raw > 0.0f)) return 0;   // an underflowed Gamma draw, also against an overflowed mu / theta (0 * inf); fminf would drop the NaN
  return nbs_poisson(st, b0, fminf(raw, NBS_LAM_MAX));
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the sampler over given parameters: out[r][g] ~ NBMix(rate_p[r][g], rate_s[r][g], theta[g], logit[r][g]); gene id = g, cell id =
// cell_ids ? cell_ids[r] : r
// ---------------------------------------------------------------------------------------------------------------------------------
struct NbMixArgs {
  const float *rate_p, *rate_s, *logit; long ld_in;
  const float* theta;
  int R, G;
  const int* cell_ids;
  unsigned long long key; unsigned sample;
  int* out; long ld_out;
};

__global__ __launch_bounds__(256) void nbmix_sample_kernel(NbMixArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)a.R * a.G) return;
  const int r = (int)(i / a.G), g = (int)(i - (long)r * a.G);
  const NbStream st{{(unsigned)a.key, (unsigned)(a.key >> 32)}, (unsigned)g, (unsigned)(a.cell_ids ? a.cell_ids[r] : r), a.sample};
  const long src = (long)r * a.ld_in + g;
  a.out[(long)r * a.ld_out + g] = nbmix_draw(st, a.rate_p[src], a.rate_s[src], a.theta[g], a.logit[src]);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// decode and draw: dec_expected_kernel's workgroup and its decode front-end, shared as code (dx_stage_am, dx_tile_gene, dx_decode_tile
// of spv_dec_expected.h); then one nbmix_draw per accumulator element in place of dx_value, and the same turn through the wave's LDS
// tile for the store.
//   * The accumulator layout is lane = cell, registers = genes: the id and theta of the tile's 32 genes, which lane r < 32 holds
//     for gene r, go through 32-entry LDS rows of the wave before the draws.
//   * The 16 draws of a lane run as a ROLLED loop (the sampler's rejection loops sixteen times over would be ~16x the code); the
//     three accumulator vectors are rotated by one register per trip, so the loop reads element 0 and indexes no register array.
//   * Elements outside the selection or beyond row B are not drawn (and never stored).
// ---------------------------------------------------------------------------------------------------------------------------------
struct DecSampleArgs {
  const bf16_t *Am_hi, *Am_lo, *Wm_hi, *Wm_lo;
  int K;
  const int* genes; int n_genes;
  const float* theta;       // [G] exp(px_r)
  const int* cell_ids;      // [B] or null
  unsigned long long key; unsigned sample;
  int* out; long ld_out; int ld_gene;
};

// A wave-uniform pointer moved into vector registers.  The draw loop's nested divergent loops hold an exec mask each and its constants
// sit in scalar registers; with the operand pointers of the decode and store stages live across it as well, the kernel needs more
// than the 102 SGPRs there are and the allocator parks the excess in VGPR lanes.  Vector registers are plentiful here.
template <typename T>
__device__ __forceinline__ T* nbs_in_vgpr(T* ptr) {
  unsigned lo = (unsigned)reinterpret_cast<uintptr_t>(ptr), hi = (unsigned)(reinterpret_cast<uintptr_t>(ptr) >> 32);
  asm volatile("" : "+v"(lo), "+v"(hi));
  return reinterpret_cast<T*>(((uintptr_t)hi << 32) | lo);
}

__device__ __forceinline__ f16v nbs_rot(const f16v& v) { return __builtin_shufflevector(v, v, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 0); }

template <int NSPLIT, int KW>
__global__ __launch_bounds__(256) void dec_sample_kernel(DecParams p, DecSampleArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t s_am[(NSPLIT == 3 ? 2 : 1) * DX_PLANE];
  __shared__ __attribute__((aligned(16))) int s_t[4][32 * DX_TPITCH];
  __shared__ int s_gid[4][32];
  __shared__ float s_th[4][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, r = lane & 31;
  const int cell0 = blockIdx.x * DX_CELLS;   // (cell0 + 32 <= Bp: the grid has Bp / 32 columns)
  const bf16_t* const wps_hi = nbs_in_vgpr(p.Wps_hi), * const wps_lo = nbs_in_vgpr(p.Wps_lo);
  dx_stage_am<NSPLIT>(s_am, a.Am_hi, a.Am_lo, a.K, cell0, tid);
  PsFragsK<KW> cf;
  load_ps_cell_frags(p, cell0, lane, cf);
  const float ap = p.a_p[cell0 + r], as = p.a_s[cell0 + r];
  const bool cell_ok = cell0 + r < p.B;
  const int cell_id = a.cell_ids ? a.cell_ids[min(cell0 + r, p.B - 1)] : cell0 + r;
  NbStream st{{(unsigned)a.key, (unsigned)(a.key >> 32)}, 0u, (unsigned)cell_id, a.sample};
  __syncthreads();
  const int ntiles = (a.n_genes + 31) >> 5;
  const bf16_t* const wm_hi = nbs_in_vgpr(a.Wm_hi), * const wm_lo = NSPLIT == 3 ? nbs_in_vgpr(a.Wm_lo) : nullptr;
  const int* const genes = a.genes ? nbs_in_vgpr(a.genes) : nullptr;
  const float* const theta = nbs_in_vgpr(a.theta);
  int* const out = nbs_in_vgpr(a.out);
  int* const tile = s_t[wave];
  const bf16_t* const arow = s_am + r * DX_APITCH + 8 * h;
  for (int t = blockIdx.y * 4 + wave; t < ntiles; t += gridDim.y * 4) {
    const int sel0 = t * 32;
    const int g = dx_tile_gene(genes, a.n_genes, sel0, r, p.G);   // (a column beyond the selection: never drawn, never stored)
    if (h == 0) { s_gid[wave][r] = g; s_th[wave][r] = theta[g]; }
    f16v yp, ys, acc;
    dx_decode_tile<NSPLIT, KW>(wps_hi, wps_lo, wm_hi, wm_lo, a.K, g, h, arow, cf, yp, ys, acc);
    dx_wave_sync();   // s_gid / s_th of this tile are visible to the wave
    // ---- draws (lane-divergent from here to the hand-over) -> the wave's LDS tile [cell r][gene crow(q, h)] ------------------
#pragma clang loop unroll(disable)
    for (int q = 0; q < 16; ++q) {
      const int gc = crow(q, h);
      if (cell_ok && sel0 + gc < a.n_genes) {
        st.gene = (unsigned)s_gid[wave][gc];
        tile[r * DX_TPITCH + gc] = nbmix_draw(st, __expf(yp[0] + ap), __expf(ys[0] + as), s_th[wave][gc], acc[0]);
      }
      yp = nbs_rot(yp); ys = nbs_rot(ys); acc = nbs_rot(acc);
    }
    dx_wave_sync();
    // ---- store with lane = gene: rows 2 i + h, 32 consecutive columns each ------------------------------------------------
    const int col = sel0 + r;
    // (rolled: unrolled, the sixteen loop-invariant row masks are hoisted out of the tile loop and cost 32 SGPRs, more than are left)
    if (col < a.n_genes) {
      const int nrow = min(p.B - cell0, 32);
#pragma clang loop unroll(disable)
      for (int c = h; c < nrow; c += 2) out[(long)(cell0 + c) * a.ld_out + (long)col * a.ld_gene] = tile[c * DX_TPITCH + r];
    }
    dx_wave_sync();   // the tile and the gene rows are rewritten by the next iteration
  }
}

}  // namespace spv
