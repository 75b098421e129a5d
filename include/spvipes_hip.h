/* spvipes_hip.h -- C ABI of the MI355X (gfx950) hot-path library  libspvipes_hip.so
 *
 * Drop-in boundary for the per-minibatch VAE step of nrclaudio/spVIPES.  The reference has no
 * native code and no FFI of its own: its hot path is a sequence of stock torch ops inside
 * src/spVIPES/module/spVIPESmodule.py and src/spVIPES/nn/networks.py.  Each entry point below
 * names the reference lines whose arithmetic it replaces; spvipes_amd/_abi.py is the ctypes
 * binding, INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless marked host; no allocation happens inside
 *     (workspaces are passed in); every call only enqueues work on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream) and returns immediately;
 *   - return value: SPV_OK (0) or a negative SPV_ERR_*; spv_last_error() gives the text;
 *   - thread-compatible, not thread-safe; no exceptions cross the ABI;
 *   - "bf16" = raw 16-bit words (uint16_t).  Packed operand images are zero padded by
 *     spv_pack_bf16 so that whole tiles are always in bounds;
 *   - precision mode `nsplit`: 1 = bf16 operands, fp32 accumulate;
 *                              3 = split-bf16 (hi/lo) operands, ~fp32 products ("fp32" mode).
 */
#ifndef SPVIPES_HIP_H
#define SPVIPES_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPV_OK 0
#define SPV_ERR_ARG (-1)
#define SPV_ERR_LAUNCH (-2)
#define SPV_ERR_UNSUPPORTED (-3)

#define SPV_COUNT_F32 0
#define SPV_COUNT_U16 1

#define SPV_NB_CMAX 64      /* rows of the (count, gene) lgamma/digamma table         */
#define SPV_DEC_KP 16       /* K slots of the private factor regressor (n_p + 1 <= 16) */
#define SPV_DEC_KS 32       /* K slots of the shared factor regressor  (n_s + 1 <= 32) */
#define SPV_DEC_KP_WIDE 32  /* the wide operand layout (kslots = 1 in spv_dec_params, spv_zsplit_args, spv_fold_batch): n_p + 1 <= 32 */
#define SPV_DEC_KS_WIDE 64  /*                                                                                          n_s + 1 <= 64 */
#define SPV_DEC_CELLS_PER_WG 128

int spv_version(void);
const char* spv_last_error(void);
/* Fingerprint (32 hex digits) of the sources and compiler flags this library was built from; the Python binding refuses a
 * library whose fingerprint differs from the sources next to it (spvipes_amd/build.py: build_id). */
const char* spv_build_id(void);

/* Count matrix of one group: X[cell][gene], row-major, resident in HBM.
 * rows == NULL means "cells 0..B-1"; otherwise cell b of the minibatch is row rows[b]
 * (the AnnDataLoader row gather, dataloaders/_ann_dataloader.py, fused into the kernels).
 * col_off selects the group's own genes inside an outer-joined matrix
 * (x[:, groups_var_indices[g]], module/spVIPESmodule.py:428-430). */
typedef struct spv_counts {
  const void* X;
  int64_t ld;       /* elements per row                    */
  const int32_t* rows;
  int32_t col_off;
  int32_t dtype;    /* SPV_COUNT_F32 | SPV_COUNT_U16       */
} spv_counts;

/* fp32 [R][C] (+ one optional extra column: a per-row vector, or the constant 1) -> bf16 hi (and
 * lo = bf16(x - hi) when dst_lo != NULL) image dst[Rp][ld_dst], written at column dst_col_off
 * over `cslot` columns and `Rp` rows, zero filled outside the source. */
int spv_pack_bf16(const float* src, int64_t ld_src, int32_t R, int32_t C,
                  const float* extra_col, int32_t extra_one,
                  uint16_t* dst_hi, uint16_t* dst_lo, int64_t ld_dst, int32_t dst_col_off,
                  int32_t Rp, int32_t cslot, void* stream);

/* The encoder's first layer in the nsplit == 1 mode keeps its 16-bit operand images as IEEE f16 words (11 significant bits instead
 * of bf16's 8, same MFMA rate; a 10 000 .. 30 000-term contraction with bf16 operands left the latent means 5e-3 off the fp32
 * reference): the weight image W1_hi = f16(W * spv_fc1_w_scale()) (a power of two, undone by the forward epilogue), the resident
 * log1p image of spv_prepare_log1p, and the dh image of the weight gradient scaled per step by a power of two (spv_enc_fc1_bwd_prep).
 * spv_pack_f16: fp32 [R][C] * scale -> f16 image dst[Rp][ld_dst] over `cslot` columns, zero filled outside the source, saturating
 * (cslot and ld_dst multiples of 8, dst 16-byte aligned). */
float spv_fc1_w_scale(void);
int spv_pack_f16(const float* src, int64_t ld_src, int32_t R, int32_t C, uint16_t* dst, int64_t ld_dst, int32_t Rp, int32_t cslot,
                 float scale, void* stream);

/* 1 when spv_enc_fc1_fwd will take its LDS-DMA kernel for these shapes (resident bf16 log1p image, N1 = 256, nsplit 1, operand rows
 * zero padded to multiples of 64 genes).  The caller needs to know because that path wants `slabs` sized
 * [splits][round_up(B, 128)][N1] fp32 (it keeps the partial sums in MFMA accumulator-tile order) and splits chosen as
 * clamp(256 / ceil(B / 128), 1, 16) with at least four 64-gene steps per split. */
int spv_enc_fc1_fwd_uses_dma(int32_t B, int32_t G, int32_t N1, int32_t nsplit, int32_t have_xb, int64_t ldw, int64_t ld_xb);

/* A1 + first layer of both encoders of a group (module/spVIPESmodule.py:428-435,
 * nn/networks.py:119):  h1 = relu(log1p(X[rows]) @ W1^T + b1) for the concatenated
 * [private ; shared] fc1 (N1 = 2 * n_hidden output columns), library = log(sum_g log1p(x)).
 *   W1_hi/lo : [N1p][ldw] (rows = output units, K = genes contiguous, ldw % 32 == 0): nsplit 3: bf16 hi / lo of W;
 *              nsplit 1: W1_hi = f16(W * spv_fc1_w_scale()) from spv_pack_f16 / spv_adam_step_images, W1_lo unused
 *   bias     : fp32 [N1], or the two encoders' biases in place: bias [n_first] and bias2 [N1 - n_first]
 *              (bias2 == NULL: one vector)
 *   slabs    : fp32 workspace [splits][B][N1];  rowsum_ws: fp32 [splits][B]
 *   h1       : fp32 [B][N1];  library: fp32 [B]
 *   xb_all, library_all : optional (nsplit 1 only): f16(log1p(x)) of the WHOLE resident count matrix [n_cells][ld_xb] (zero
 *              padded to ld_xb >= round_up(G, 128)) and log(sum_g log1p(x)) per cell, both from spv_prepare_log1p; the GEMM
 *              then gathers plain bf16 rows through x->rows instead of decoding counts, and library is a table lookup
 *   cov, cov_idx : optional (both or neither): one-hot batch covariates appended to the layer's input (nn/networks.py:105-119,
 *              module/spVIPESmodule.py:133,440-445) as what they amount to: cov fp32 [n_batch][N1] = the weight columns of the
 *              covariates, transposed, both encoders side by side; cov_idx int32 [B] = the batch code of every minibatch cell;
 *              cov[cov_idx[b]][:] is added before the ReLU */
int spv_enc_fc1_fwd(const spv_counts* x, int32_t B, int32_t G,
                    const uint16_t* W1_hi, const uint16_t* W1_lo, int64_t ldw, int32_t N1,
                    const float* bias, const float* bias2, int32_t n_first, int32_t nsplit, int32_t splits,
                    float* slabs, float* rowsum_ws, float* h1, float* library,
                    const uint16_t* xb_all, int64_t ld_xb, const float* library_all,
                    const float* cov, const int32_t* cov_idx, void* stream);

/* Once per resident count matrix: xb[c][g] = f16(log1p(X[c][g])) (zero for g >= G, row pitch ld_xb) and
 * library[c] = log(sum_g log1p(X[c][g])) (module/spVIPESmodule.py:428-435 evaluated for every cell of the data set).
 * x->rows is ignored.                                                                                               */
int spv_prepare_log1p(const spv_counts* x, int32_t n_cells, int32_t G, uint16_t* xb, int64_t ld_xb, float* library, void* stream);
/* The same for the "fp32" (nsplit 3) mode: bf16 hi words of log1p(x) and lo words (bf16(x - hi)), interleaved in blocks of 32 genes --
 * words [64 b, 64 b + 32) of a row are the hi words of genes 32 b .. 32 b + 31, words [64 b + 32, 64 b + 64) their lo words (one
 * 128-byte line = what one K tile of the LDS-DMA fc1 kernel takes from a row); ld_xb (words per row) a multiple of 128,
 * >= 2 round_up(G, 64) for that kernel, zero padded.  spv_enc_fc1_fwd takes it as xb_all with nsplit 3 and that ld_xb. */
int spv_prepare_log1p_split(const spv_counts* x, int32_t n_cells, int32_t G, uint16_t* xb, int64_t ld_xb, float* library, void* stream);

/* Count matrix of one group resident in HBM as CSR, densified per minibatch (replaces the AnnTorchDataset row densification of
 * dataloaders/_ann_dataloader.py for a sparse AnnData.X, plus the slice / log1p / library of module/spVIPESmodule.py:428-435).
 * Writes exactly the bytes the dense-resident path hands the downstream kernels, so that spv_enc_fc1_*, the likelihood's
 * spv_dec_params (X, ldx, rows) and the pair grids then run on the minibatch buffers with rows = 0..B-1:
 *   X       : [B][ldx] counts of cells rows[0..B) in the value dtype, zero where a gene has no stored entry (and for g >= G);
 *             ldx >= G, a multiple of 8; 16-byte aligned
 *   xb      : optional: xb_split 0: the f16 image of spv_prepare_log1p ([B][ld_xb], ld_xb >= G, a multiple of 8);
 *             xb_split 1: the interleaved hi / lo image of spv_prepare_log1p_split (ld_xb a multiple of 128, >= 2 round_up(G, 32));
 *             bit-identical to those entries' rows rows[b], padding included; 16-byte aligned
 *   library : [B] log(sum_g log1p(x)) in the summation order of those entries (bit-identical); required with xb, else optional
 * CSR: indptr int64 [n_rows + 1] (more than 2^31 stored entries are fine), cols int32 [nnz] local gene indices in [0, G), sorted and
 * unique within a row, vals [nnz] uint16 or fp32 (dtype).  A row index outside [0, n_rows) reads as an empty row.  Every group of
 * the call runs in one grid; nothing is allocated and the row indices are read on the device (graph capture safe). */
#define SPV_CSR_GATHER_MAXG 8
typedef struct spv_csr_gather_args {
  const int64_t* indptr;
  const int32_t* cols;
  const void* vals;
  int32_t n_rows;
  int32_t G;
  int32_t dtype;       /* SPV_COUNT_F32 | SPV_COUNT_U16 (of vals and X) */
  int32_t B;
  const int32_t* rows; /* [B] */
  void* X;
  int64_t ldx;
  uint16_t* xb;
  int64_t ld_xb;
  int32_t xb_split;
  int32_t pad_;
  float* library;
} spv_csr_gather_args;
int spv_csr_gather(const spv_csr_gather_args* groups, int32_t n_groups, void* stream);

/* fc1 weight gradient (autograd of nn/networks.py:119):  dW1[N1][G] = dh^T @ log1p(X[rows]).
 *   dh_hi/lo : [round_up(B,64)][ld_dh] (ld_dh >= round_up(N1,128), zero padded) from spv_enc_fc1_bwd_prep: nsplit 3 bf16 hi / lo,
 *              nsplit 1 f16(dpre * scale) with dh_scale = that call's scale_ws ({scale, 1 / scale}: the result is multiplied by [1])
 *   xb       : optional: nsplit 1: the resident f16 log1p image of spv_prepare_log1p ([n_cells][ld_xb], gathered through x->rows);
 *              nsplit 3: the resident split image of spv_prepare_log1p_split, where spv_enc_fc1_wgrad_split_uses_dma says so
 *              (B <= 4096-ish: the row-index table of the minibatch sits in LDS); NULL = decode the counts here
 *   dW2      : optional second destination: rows >= rows_first go to dW2[row - rows_first] (the shared
 *              encoder's weight gradient, stored apart from the private encoder's)  */
int spv_enc_fc1_wgrad_split_uses_dma(int32_t B, int32_t G, int32_t N1, int64_t ld_dh, int64_t ld_xb);   /* nsplit 3: may xb be passed? */
int spv_enc_fc1_wgrad(const spv_counts* x, int32_t B, int32_t G,
                      const uint16_t* dh_hi, const uint16_t* dh_lo, int64_t ld_dh, int32_t N1,
                      int32_t nsplit, float* dW, float* dW2, int32_t rows_first, int64_t ldc,
                      const uint16_t* xb, int64_t ld_xb, const float* dh_scale, void* stream);

/* Backward of fc1's ReLU + bias (nn/networks.py:119): dpre = dh1 * (h1 > 0) packed as the 16-bit image
 * spv_enc_fc1_wgrad consumes ([Bp][ld_img], zero padded), and the bias gradients
 * db[col] = sum_b dpre[b][col] (cols >= n_first to db2[col - n_first] when db2 != NULL).
 *   img_lo != NULL ("fp32" mode): bf16 hi / lo images;  img_lo == NULL: img_hi = f16(dpre * scale), scale = the power of two that
 *   brings max |dpre| of this call into [4096, 8192) (a pure function of dpre: no state across steps, no atomics)
 *   part     : fp32 workspace [Bp / 16][N1]
 *   scale_ws : fp32 [2 + Bp / 16] (required when img_lo == NULL): [0] = scale, [1] = 1 / scale, rest = per-block maxima */
int spv_enc_fc1_bwd_prep(const float* dh1, const float* h1, int32_t B, int32_t N1, uint16_t* img_hi, uint16_t* img_lo,
                         int64_t ld_img, int32_t Bp, float* part, float* db, float* db2, int32_t n_first, float* scale_ws, void* stream);

/* Grouped forms of the three fc1 entry points above: one argument block per group (same meaning as the parameters of
 * spv_enc_fc1_fwd / spv_enc_fc1_bwd_prep + spv_enc_fc1_wgrad).  Pairs of groups whose shapes take the LDS-DMA kernels run as ONE launch
 * per kernel (both groups' tiles in one grid: the 2 x 256 one-per-CU workgroups of two separate launches can only run one after the
 * other anyway, and a single stream needs no fork / join); anything else falls back to the per-group entry points in order. */
typedef struct spv_fc1_fwd_args {
  const spv_counts* x; int32_t B, G;
  const uint16_t* W1_hi; const uint16_t* W1_lo; int64_t ldw; int32_t N1;
  const float* bias; const float* bias2; int32_t n_first, nsplit, splits;
  float* slabs; float* rowsum_ws; float* h1; float* library;
  const uint16_t* xb_all; int64_t ld_xb; const float* library_all;
  const float* cov; const int32_t* cov_idx;   /* optional batch covariates (see spv_enc_fc1_fwd) */
} spv_fc1_fwd_args;
int spv_enc_fc1_fwd_grouped(const spv_fc1_fwd_args* groups, int32_t n_groups, void* stream);

typedef struct spv_fc1_bwd_args {
  const float* dh1; const float* h1; const spv_counts* x;
  int32_t B, G, N1, n_first, nsplit, Bp;
  uint16_t* dh_hi; uint16_t* dh_lo; int64_t ld_dh;      /* workspace: packed 16-bit image of relu'(h1) * dh1, [Bp][ld_dh] */
  float* part;                                          /* workspace: [Bp / 16][N1] column partial sums */
  float* db; float* db2; float* dW; float* dW2; int64_t ldc;
  const uint16_t* xb; int64_t ld_xb;
  float* scale_ws;                                      /* workspace: [2 + Bp / 16] (nsplit 1: scale record of the f16 dh image) */
} spv_fc1_bwd_args;
int spv_enc_fc1_bwd_grouped(const spv_fc1_bwd_args* groups, int32_t n_groups, void* stream);

/* "Accumulator-tile" order of the [cells][genes] arrays exchanged between the decoder kernels
 * (mixing logits, dL, tP, tS):  T[cell/32][gene/32][qq][lane][j], lane = cell%32 + 32 h,
 * gene%32 = 8 qq + 4 h + j, qq, j = 0..3 -- each 32x32 tile is stored as the MFMA accumulator that
 * produced it (genes on MFMA rows, register 4 qq + j), register-group major, so one wave
 * instruction moves 512 contiguous bytes.  n_gene_tiles = Gp / 32. */

/* 1 when spv_gemm_bf16 will take its LDS-DMA kernel (spvipes_amd/csrc/spv_dec_gemm.h) for these arguments: nsplit 1, a tile-ordered
 * A operand, 32 < N <= 320, ldb == 320.  It works on 128-row x 320-column workgroup tiles, so the caller should pick `splits`
 * with ceil(M / 128) * splits close to (a multiple of) the 256 CUs, and the tiled array must cover round_up(M, 128) rows /
 * round_up(K, 64) contraction indices (the decoder's Bp / Gp paddings do). */
int spv_gemm_bf16_uses_dma(int32_t a_kmajor, int32_t M, int32_t N, int32_t K, int32_t nsplit, int32_t a_tiles, int64_t ldb);

/* Plain bf16 MFMA GEMM, fp32 out:  C[M][N] (+)= sum_k A(m,k) B(k,n).
 *   a_kmajor == 0: A is mem[m][k] (k contiguous); a_kmajor == 1: A is mem[k][m];
 *   a_tiles > 0: A is a tiled [cells][genes] array (above) with a_tiles gene tiles per cell tile;
 *                a_kmajor then says whether K runs over cells (1) or over genes (0); lda is unused.
 *   B is always k-major: mem[k][n].   Operands zero padded to tile multiples: K to a multiple of 64 in both; M to a multiple
 *   of 128 where N <= 32 or spv_gemm_bf16_uses_dma() says 1, of 64 otherwise; the columns of B to 32 from the given pointer
 *   where N <= 32 (they may hold other finite data: only columns < N are stored), to a multiple of 320 otherwise.  Nothing
 *   beyond those extents is read (tests/test_gpu_gemm_family.py surrounds every operand with NaN words).
 *   splits > 1: C is a stack of `splits` fp32 slabs (slab_stride elements apart), one per K range of
 *   ceil(ceil(K / 64) / splits) * 64 indices; a trailing split whose range starts at or beyond K writes a slab of zeros and
 *   reads nothing. */
int spv_gemm_bf16(int32_t a_kmajor, const uint16_t* A_hi, const uint16_t* A_lo, int64_t lda,
                  const uint16_t* B_hi, const uint16_t* B_lo, int64_t ldb,
                  float* C, int64_t ldc, int32_t M, int32_t N, int32_t K,
                  int32_t nsplit, int32_t splits, int64_t slab_stride, int32_t a_tiles, void* stream);

/* The same GEMM with its split-K slabs summed INSIDE the launch (only where spv_gemm_bf16_uses_dma() says 1; else SPV_ERR_UNSUPPORTED):
 * every workgroup stores its slab tile, releases it (agent scope) and takes a ticket on its row tile's counter; the workgroup that draws
 * the last ticket acquires, adds the `splits` slabs of the tile IN SLAB ORDER (for splits <= 8 what spv_reduce_slabs produces, bit for bit), scales
 * by *alpha and writes columns [0, n0) to dst0 and columns [c1, c1 + n1) to dst1 -- the separate reduction launch and its re-read of the
 * slabs from HBM are gone (the decoder backward's d A_m: 2 x 21 MB per step at B 4096, on the critical chain).
 * counters: uint32 [ceil(M / 128)], ZERO when the call is made; the call leaves them zero (the last arriver resets its counter). */
typedef struct spv_gemm_fixup {
  uint32_t* counters;
  const float* alpha;                          /* device scalar, or NULL = 1                        */
  float* dst0; int64_t ld0; int32_t n0;        /* columns [0, n0) of the summed C                    */
  float* dst1; int64_t ld1; int32_t c1, n1;    /* columns [c1, c1 + n1) (dst1 == NULL: none)         */
} spv_gemm_fixup;
int spv_gemm_bf16_fix(int32_t a_kmajor, const uint16_t* A_hi, const uint16_t* A_lo, int64_t lda,
                      const uint16_t* B_hi, const uint16_t* B_lo, int64_t ldb,
                      float* C, int64_t ldc, int32_t M, int32_t N, int32_t K,
                      int32_t nsplit, int32_t splits, int64_t slab_stride, int32_t a_tiles, const spv_gemm_fixup* fix, void* stream);

/* spv_gemm_bf16 for the two groups of a step in ONE grid (group = blockIdx.y) where both calls take the bf16 LDS-DMA kernel in the same
 * direction; otherwise, and for an odd group left over, the per-group entry point in order.  Same arguments, same slabs. */
typedef struct spv_gemm_args {
  int32_t a_kmajor; int32_t pad0_;
  const uint16_t* A_hi; const uint16_t* A_lo; int64_t lda;
  const uint16_t* B_hi; const uint16_t* B_lo; int64_t ldb;
  float* C; int64_t ldc; int32_t M, N, K, nsplit, splits, a_tiles; int64_t slab_stride;
} spv_gemm_args;
int spv_gemm_bf16_grouped(const spv_gemm_args* groups, int32_t n_groups, void* stream);

/* Weight gradients of both rate heads' regressors (BatchNorm folded) in one streaming pass, bf16 mode:
 *   slabP[split][g][0..15] = sum_{cells of the split} tP(cell, g) * Aps[cell][0..15]
 *   slabS[split][g][0..31] = sum_{cells of the split} tS(cell, g) * Aps[cell][16..47]        (backward of nn/networks.py:314-320)
 * tP / tS: bf16 [Bp][Gp] in accumulator-tile order (a_tiles = Gp / 32 >= round_up(G, 128) / 32: the kernel walks 128-gene tiles; the
 * decoder's Gp = round_up(G, 256) covers that), already softmax-corrected (spv_dec_softmax_bwd); Aps: bf16 [Bp][48] latent operand
 * image; Bp % 64 == 0.  `splits` may exceed Bp / 64: a split without cells writes a slab of zeros and reads nothing.  Sum the slabs
 * with spv_reduce_slabs. */
int spv_dec_heads_wgrad(const uint16_t* tP, const uint16_t* tS, int32_t a_tiles, const uint16_t* Aps, int32_t G, int32_t Bp,
                        int32_t splits, float* slabP, float* slabS, void* stream);

/* Mixing logits of the decoder (nn/networks.py:322-325 with the bias folded into a ones column):
 *   out(b, g) = sum_k Am[b][k] * Wm[g][k],  Am bf16 [Bp][K], Wm bf16 [Gp][K], K % 32 == 0,
 *   Bp, Gp multiples of 128; out is f16 (out_f32 == 0) or f32 in accumulator-tile order. */
int spv_dec_logits(const uint16_t* Am_hi, const uint16_t* Am_lo, const uint16_t* Wm_hi, const uint16_t* Wm_lo,
                   int32_t K, int32_t Bp, int32_t Gp, int32_t nsplit, void* out, int32_t out_f32, void* stream);

/* Decoder + NB-mixture likelihood (nn/networks.py:314-325, module/spVIPESmodule.py:758-759,
 * :817-824).  Field meanings are documented in spvipes_amd/csrc/spv_decoder.h (DecParams has
 * exactly this layout). */
typedef struct spv_dec_params {
  const void* X; int64_t ldx; const int32_t* rows; int32_t col_off; int32_t count_is_u16;
  int32_t B, G, Bp, Gp;
  const void* logits; int32_t n_gene_tiles; int32_t logits_f32; /* tiled mixing logits, f16 | f32 (see below) */
  const uint16_t* Wps_hi; const uint16_t* Wps_lo;
  const uint16_t* Aps_hi; const uint16_t* Aps_lo;
  const void* gene_tab;      /* float4 [Gp]              */
  const void* cnt_tab;       /* float2 [SPV_NB_CMAX][Gp] */
  const float* a_p; const float* a_s; const float* lse_p; const float* lse_s;
  const float* w_row;
  int32_t gene_splits; int32_t genes_per_split;
  float* part_max_p; float* part_sum_p; float* part_max_s; float* part_sum_s;
  float* rec_part; float* tp_part; float* ts_part;
  float* dtheta_part;
  void* dL; void* tP; void* tS; int32_t grads_f32;              /* tiled like logits; bf16 [Bp][Gp], or (grads_f32) a bf16 hi plane
                                                                  followed by a bf16 lo plane, [2][Bp][Gp]: value = hi + lo */
  int32_t nb_splits; int32_t nb_genes_per_split;               /* gene splits of spv_dec_nb_fwd: multiple of 32, <= SPV_NB_GSPL_MAX */
  int32_t nb_cell_tiles;   /* 64-cell tiles one likelihood workgroup walks (0 = 1); dtheta_part then holds ceil(Bp / 64 / nb_cell_tiles) rows */
  int32_t kslots;          /* operand layout of Wps / Aps: 0 = 16 / 32 K slots, rows of 48; 1 = 32 / 64 K slots, rows of 96 (spv_dec_lse,
                              spv_dec_nb_fwd, spv_dec_materialize and the in-place spv_dec_softmax_bwd; the fused backward passes take 0 only) */
} spv_dec_params;

/* theta = exp(px_r) and the per-(count, gene) lgamma / digamma table (module/spVIPESmodule.py:758
 * and the lgamma terms of scvi-tools' log_mixture_nb). */
int spv_dec_tables(const float* px_r, int32_t G, int32_t Gp, void* gene_tab, void* cnt_tab, void* stream);

/* softmax denominators of both rate heads; writes lse_p/lse_s and a_k = library - lse_k
 * (the cast away of const on those four pointers is deliberate: they are this call's outputs). */
int spv_dec_lse(const spv_dec_params* p, const float* library, void* stream);

/* rec_part/tp_part/ts_part [nb_splits][Bp], dtheta_part [Bp/64][Gp]; when train != 0 also the
 * per-element gradients dL, tP, tS (accumulator-tile order; bf16, or bf16 hi + lo planes when grads_f32). */
int spv_dec_nb_fwd(const spv_dec_params* p, int32_t train, void* stream);

/* The decoder's per-group launches for the two groups of a step in ONE grid each (group = blockIdx.z; csrc/spv_decoder.h *_pair_kernel):
 * workgroups outside a group's own grid extent leave at once, the others run the single-group kernel body unchanged -- the results are
 * bit-identical to the per-group calls.  A pair goes out as one grid where both groups take the same kernel variant (count storage,
 * logits and gradient word types; bf16 LDS-DMA logits GEMM; bf16 words for the one-pass backward); otherwise, and for an odd group left
 * over, the per-group entry points run in order.  Each entry point reads the fields of spv_dec_group its per-group twin takes as arguments:
 *   spv_dec_tables_grouped   px_r  (writes p.gene_tab / p.cnt_tab)              spv_dec_logits_grouped   Am_*, Wm_*, K, nsplit (writes p.logits)
 *   spv_dec_lse_grouped      library                                            spv_dec_nb_fwd_grouped   --
 *   spv_dec_heads_bwd_grouped  Tp, Ts, dz_part, dw_part
 * At 128 cells per minibatch a likelihood launch is ~15 us of fixed cost: one grid instead of two per kernel is what shortens the step. */
typedef struct spv_dec_group {
  spv_dec_params p;
  const float* library;
  const float* px_r;
  const uint16_t* Am_hi; const uint16_t* Am_lo; const uint16_t* Wm_hi; const uint16_t* Wm_lo; int32_t K, nsplit;
  const float* Tp; const float* Ts; float* dz_part; float* dw_part;
} spv_dec_group;
int spv_dec_tables_grouped(const spv_dec_group* groups, int32_t n_groups, void* stream);
int spv_dec_logits_grouped(const spv_dec_group* groups, int32_t n_groups, void* stream);
int spv_dec_lse_grouped(const spv_dec_group* groups, int32_t n_groups, void* stream);
int spv_dec_nb_fwd_grouped(const spv_dec_group* groups, int32_t n_groups, int32_t train, void* stream);
int spv_dec_heads_bwd_grouped(const spv_dec_group* groups, int32_t n_groups, void* stream);

/* Materialises the decoder outputs the reference's generative() returns (module/spVIPESmodule.py:751-768,
 * nn/networks.py:314-325) for one group: px_scale_k = softmax_G(BN(z_k W_k^T)), px_rate_k = exp(library) * px_scale_k
 * (k = private, shared) and the mixing logits, as row-major fp32 [B][ld] (ld >= G).  Off the hot path: the fused
 * likelihood (spv_dec_nb_fwd) never stores them.  Needs spv_dec_logits and spv_dec_lse to have run on `p`. */
int spv_dec_materialize(const spv_dec_params* p, float* scale_private, float* scale_shared, float* rate_private, float* rate_shared,
                        float* mixing_logits, int64_t ld, void* stream);

/* Denoised-expression read-out over a selected list of genes (get_normalized_expression): for one group and one minibatch, ONE
 * row-major fp32 array out[B][ld_out] of the NB mixture's mean or of one of its ingredients (nn/networks.py:314-325,
 * module/spVIPESmodule.py:751-759; pi = sigmoid(mixing logits) weights component 1, the private rate):
 *   what = 0  pi * rate_private + (1 - pi) * rate_shared      1  pi * rate_private      2  (1 - pi) * rate_shared      3  pi
 *   out[b][j] = alpha * value(b, genes[j])   or, with accumulate != 0,   out[b][j] += alpha * value(b, genes[j])
 * `p` is the operand set as spv_dec_lse leaves it (Wps, Aps, a_p / a_s = library - lse over ALL G genes, either kslots layout; hand
 * spv_dec_lse a library vector filled with log L for a fixed library size L).  Am / Wm are the mixing operands spv_dec_logits takes
 * (bf16 [Bp][K] / [Gp][K], bias in the ones column, lo planes when nsplit == 3; K % 32 == 0, K <= 320, 16-byte aligned): the logits
 * of the selected genes are accumulated inside the kernel, p->logits is not read.  genes: int32 device array of n_genes ids in
 * [0, G), any order, repeats allowed (ids outside the range are clamped into it, never dereferenced out of bounds); NULL = genes
 * 0 .. n_genes - 1 (n_genes <= G).  An element's value depends on its own gene and cell only: the output over a selection equals
 * the same columns of the all-genes output bit for bit, and its rates equal spv_dec_materialize's.  Rows >= B and columns >= n_genes
 * of `out` are never written.  Nothing is allocated; one launch on `stream`. */
typedef struct spv_dec_expected_args {
  const uint16_t* Am_hi; const uint16_t* Am_lo; const uint16_t* Wm_hi; const uint16_t* Wm_lo;
  int32_t K, nsplit;
  const int32_t* genes; int32_t n_genes; int32_t what;
  float* out; int64_t ld_out;
  float alpha; int32_t accumulate;
} spv_dec_expected_args;
int spv_dec_expected(const spv_dec_params* p, const spv_dec_expected_args* a, void* stream);

/* Posterior-predictive counts (posterior_predictive_sample): for one group and one minibatch, one draw per (cell, selected gene) from
 * the decoder's NB mixture, NegativeBinomialMixture(mu1 = rate_private, mu2 = rate_shared, theta1 = exp(px_r), mixture_logits) of
 * module/spVIPESmodule.py:751-759 (no theta2: both components share theta), sampled as scvi-tools samples it:
 *   c ~ Bernoulli(pi), pi = sigmoid(mixing logit) weights component 1 (the private rate);  mu = c ? rate_private : rate_shared;
 *   lam = Gamma(shape = theta, scale = mu / theta) clamped at 1e8;  x ~ Poisson(lam)
 *   out[b * ld_out + j * ld_gene] = x(b, genes[j])      (int32; ld_gene >= 1, ld_out >= (n_genes - 1) * ld_gene + 1)
 * `p`, Am / Wm, K, nsplit, genes / n_genes: exactly as spv_dec_expected takes them -- the rates and the logit of an element are the
 * values that entry point computes.  theta: fp32 device array [G] of exp(px_r).  The random bits of an element are Philox 4x32-10
 * blocks addressed by (key; gene id, cell id, sample, block number), cell id = cell_ids ? cell_ids[b] : b (int32 device array [B]):
 * a value depends on its own gene, cell, sample and key only, so a gene subset equals the same columns of the all-genes output bit
 * for bit, and [B][n_genes][S] is filled in place by S calls with sample = s, out + s, ld_gene = S.  Rows >= B, columns >=
 * n_genes and the elements between the ld_gene strides are never written.  Nothing is allocated; one launch on `stream`. */
typedef struct spv_dec_sample_args {
  const uint16_t* Am_hi; const uint16_t* Am_lo; const uint16_t* Wm_hi; const uint16_t* Wm_lo;
  int32_t K, nsplit;
  const int32_t* genes; int32_t n_genes; int32_t ld_gene;
  const float* theta;
  const int32_t* cell_ids;
  uint64_t key; uint32_t sample;
  int32_t* out; int64_t ld_out;
} spv_dec_sample_args;
int spv_dec_sample(const spv_dec_params* p, const spv_dec_sample_args* a, void* stream);

/* Posterior-predictive check (posterior_predictive_check): spv_dec_sample's draws for one group and one minibatch, reduced inside the
 * kernel instead of stored.  `p`, Am / Wm, K, nsplit, genes / n_genes, theta, cell_ids, key, sample: exactly as spv_dec_sample takes
 * them (NegativeBinomialMixture of module/spVIPESmodule.py:751-759) -- x(b, genes[j]) is the integer that entry point would write.
 *   seg: int32 device array [B] of segment codes in [0, n_seg), or NULL for everything in segment 0; a cell with a negative code
 *        (and one with a code >= n_seg) is neither drawn nor counted.
 *   stats: uint64 device array [n_seg][4][ld_stats], ld_stats >= n_genes; over the counted cells b of segment k
 *        stats[k][0][j] += sum x      stats[k][1][j] += #(x > 0)      stats[k][2][j] += sum x^2 (modulo 2^64)
 *        stats[k][3][j]  = max(stats[k][3][j], max x)
 *   cell_total: uint64 device array [B] or NULL; cell_total[b] += sum_j x(b, genes[j]) for every counted cell.
 * Everything ACCUMULATES: the caller zeroes the arrays once, and one table then collects every sample of every minibatch of a walk.
 * The updates are 64-bit integer atomics, so the tables equal the reduction of spv_dec_sample's output bit for bit, in any order of
 * calls, and two runs agree bit for bit.  Columns >= n_genes, rows of segments no counted cell belongs to and cell_total entries of
 * cells that are not counted are never touched; a repeated gene of the selection fills its own column.  Nothing of size cells x
 * genes is written.  Nothing is allocated; one launch on `stream`. */
typedef struct spv_dec_sample_stats_args {
  const uint16_t* Am_hi; const uint16_t* Am_lo; const uint16_t* Wm_hi; const uint16_t* Wm_lo;
  int32_t K, nsplit;
  const int32_t* genes; int32_t n_genes; int32_t n_seg;
  const float* theta;
  const int32_t* cell_ids;
  uint64_t key; uint32_t sample;
  const int32_t* seg;
  uint64_t* stats; int64_t ld_stats;
  uint64_t* cell_total;
} spv_dec_sample_stats_args;
int spv_dec_sample_stats(const spv_dec_params* p, const spv_dec_sample_stats_args* a, void* stream);

/* Expected-expression statistics (expression_statistics): spv_dec_expected's values for one group and one minibatch (the NB mixture
 * of nn/networks.py:314-325 and module/spVIPESmodule.py:751-759), reduced over the cells of each segment instead of stored.
 * `p`, Am / Wm, K, nsplit, genes / n_genes: exactly as spv_dec_expected takes them; with
 * v_w(b, j) the fp32 value that entry point writes for what = w (0 mixture mean, 1 private part, 2 shared part, 3 mixing weight) at
 * alpha = 1, bit for bit,
 *   stats[k][w][j] += sum of v_w(b, genes[j])        stats[k][4 + w][j] += sum of v_w(b, genes[j])^2        (w = 0 .. 3)
 * over the counted cells b of segment k.  stats: fp64 device array [n_seg][8][ld_stats], ld_stats >= n_genes.  Every value is widened
 * to fp64 before it is added and its square is formed in fp64 (exact).
 * The cells arrive arranged by segment, in tiles of 32 consecutive operand rows:
 *   tile_seg: int32 device array [Bp / 32]: the segment of tile t; a negative code or a code >= n_seg skips the whole tile.
 *   tile_n:   int32 device array [Bp / 32]: the first tile_n[t] rows of tile t count (values above 32 mean 32, values <= 0 skip the
 *             tile); the other rows of the tile and rows >= B are padding and are never counted.  Entries of tiles that lie wholly at
 *             or beyond row B are not read.
 *   ws:       fp64 device scratch of spv_dec_expected_stats_ws_bytes(n_genes, Bp / 32) bytes = [Bp / 32][8][n_genes]: a workgroup
 *             per counted tile writes the tile's eight partial sums per gene, a second kernel of the same call adds them onto `stats`
 *             tile after tile in ascending order (one writer per table element).
 * Everything ACCUMULATES: the caller zeroes `stats` once, and one table collects a whole walk.  There are no floating-point atomics
 * and the order of every addition is fixed by (B, tile_seg, tile_n): two calls agree bit for bit.  Columns >= n_genes, rows of
 * segments no counted tile belongs to and everything beyond ws_bytes are never touched; a repeated gene of the selection fills its
 * own column.  Nothing is allocated; two launches on `stream`. */
typedef struct spv_dec_expected_stats_args {
  const uint16_t* Am_hi; const uint16_t* Am_lo; const uint16_t* Wm_hi; const uint16_t* Wm_lo;
  int32_t K, nsplit;
  const int32_t* genes; int32_t n_genes; int32_t n_seg;
  const int32_t* tile_seg;
  const int32_t* tile_n;
  double* stats; int64_t ld_stats;
  double* ws;
} spv_dec_expected_stats_args;
int spv_dec_expected_stats(const spv_dec_params* p, const spv_dec_expected_stats_args* a, void* stream);
int64_t spv_dec_expected_stats_ws_bytes(int32_t n_genes, int32_t n_cell_tiles);

/* The same sampler over given parameters (the law of module/spVIPESmodule.py:751-759 for anyone who holds its parameters):
 *   out[r * ld_out + g] ~ NBMix(rate_p[r * ld_in + g], rate_s[r * ld_in + g], theta[g], logit[r * ld_in + g]),  r < R, g < G
 * fp32 device inputs, int32 device output; ld_in, ld_out >= G.  key / sample / cell_ids (int32 [R] or NULL = the row number) mean
 * what they mean for spv_dec_sample, with gene id = g: equal parameters give the draws of spv_dec_sample bit for bit.  An element
 * whose selected rate or whose theta is NaN, zero or negative gives 0 (both entry points). */
int spv_nbmix_sample(const float* rate_p, const float* rate_s, const float* logit, int64_t ld_in, const float* theta, int32_t R, int32_t G,
                     const int32_t* cell_ids, uint64_t key, uint32_t sample, int32_t* out, int64_t ld_out, void* stream);

/* Differential expression in "change" mode (spVIPES.differential_expression): per gene j < n_genes the statistics, over n_pairs
 * pairs m of bank rows, of
 *   lfc_m = log2(max(x1 + eps, FLT_MIN)) - log2(max(x2 + eps, FLT_MIN)),   x1 = bank1[rows1[m]][j],  x2 = bank2[rows2[m]][j]
 * written as seven fp32 rows of stats[7][ld_stats]:
 *   0 mean of lfc   1 its standard deviation (population form, / n_pairs)   2 its minimum   3 its maximum
 *   4 the COUNT of pairs with |lfc_m| >= delta (a whole number, exact: n_pairs <= 2^24)   5 mean of x1   6 mean of x2
 * bank1 / bank2: fp32 device arrays [n_rows][ld], ld >= n_genes; rows1 / rows2: int32 device arrays [n_pairs]; a row number outside
 * [0, n_rows) is clamped into it before it indexes anything.  log2 is the hardware's v_log_f32 (1 ulp).  Every pair's term is formed
 * in fp32; a lane sums at most ceil(ceil(n_pairs / S) / 4) of them in fp32, shifted by the chunk's first lfc (so the sums of squares
 * are those of the deviations), S = spv_de_pairs_splits(n_genes, n_pairs); everything above that is merged in fp64 with Chan's
 * pairwise formula, in a fixed order.  There are no floating-point atomics: two calls with the same inputs agree bit for bit, and a
 * constant column has std == 0 and mean == min == max exactly.  S depends on n_genes, so a gene's last bits may differ between runs
 * over different gene selections.  ws: caller's scratch of at least S * 7 * n_genes doubles (8-byte aligned), overwritten.  Columns
 * >= n_genes of `stats` are never written.  Nothing is allocated; two launches on `stream`. */
typedef struct spv_de_pairs_args {
  const float* bank1; const float* bank2; int64_t ld1, ld2;
  const int32_t* rows1; const int32_t* rows2; int32_t n_rows1, n_rows2;
  int32_t n_genes, n_pairs; float delta, eps;
  float* stats; int64_t ld_stats;
  void* ws; int64_t ws_bytes;
} spv_de_pairs_args;
int spv_de_pairs(const spv_de_pairs_args* a, void* stream);
/* the number of pair splits S spv_de_pairs uses for this shape (0 for a non-positive argument) */
int32_t spv_de_pairs_splits(int32_t n_genes, int32_t n_pairs);

/* The exact per-gene median of the same lfc_m over the same pairs (the column "lfc_median" of the user API): with the n_pairs fp32
 * values lfc_m of gene j sorted ascending, mid[0][j] = the value of rank (n_pairs - 1) / 2 and mid[1][j] = the value of rank
 * n_pairs / 2 (0-based, integer division: numpy's two middle elements, equal for odd n_pairs; the median is their mean).  Banks,
 * row arrays, clamping of row numbers, eps and 1 <= n_pairs <= 2^24 as for spv_de_pairs; every lfc_m is formed by the same fp32
 * operations, so the outputs are ELEMENTS of the multiset spv_de_pairs reduces (min <= mid[0] <= mid[1] <= max), not an
 * interpolation or a histogram estimate.  -0.0 and +0.0 count as equal (either may be returned); NaN in a bank is outside the
 * contract.  How: a radix select on the order-preserving uint32 image of the values, 8 bits per pass -- four passes that gather
 * the rows again and count, per gene, the keys under the prefix found so far (uint32 counters throughout), each followed by a
 * small per-gene bin pick; the upper middle value rides along (no pass of its own).  Nothing of size n_pairs x n_genes is stored.
 * Integer atomics only: two calls agree bit for bit.  ws: caller's scratch of at least spv_de_median_ws_bytes(n_genes, n_pairs)
 * bytes = (256 + 5) * n_genes * 4 (4-byte aligned), overwritten.  Columns >= n_genes of `mid` are never written, bank columns
 * >= n_genes never read.  Nothing is allocated; nine launches on `stream`. */
typedef struct spv_de_median_args {
  const float* bank1; const float* bank2; int64_t ld1, ld2;
  const int32_t* rows1; const int32_t* rows2; int32_t n_rows1, n_rows2;
  int32_t n_genes, n_pairs; float eps;
  float* mid; int64_t ld_mid;
  void* ws; int64_t ws_bytes;
} spv_de_median_args;
int spv_de_median(const spv_de_median_args* a, void* stream);
/* the workspace spv_de_median needs for this shape, in bytes (0 for a non-positive argument) */
int64_t spv_de_median_ws_bytes(int32_t n_genes, int32_t n_pairs);

/* Statistics of the OBSERVED counts per population (the columns raw_mean / non_zeros_proportion / raw_normalized_mean of scvi-tools'
 * differential-expression tables; spVIPES.count_statistics of the user API): a segmented column reduction over LISTED rows of a dense
 * resident count matrix.  The list has n positions; position p names the cell x.rows[p - pos_off] (x.rows == NULL: cell p - pos_off);
 * the same cell may be listed more than once, in any order.  The list is cut into slabs, contiguous ranges of positions that each
 * belong to ONE segment (label): slabs int32 [n_slabs][3] = {begin, end, segment} (positions, end exclusive, end - begin <=
 * spv_count_stats_slab() is what the host plans; up to 32768 is accepted), ascending and segment by segment, and seg_slabs int32
 * [n_seg + 1]: segment k owns slabs [seg_slabs[k], seg_slabs[k + 1]) (none: an empty segment, which yields zeros).  For segment k
 * and selected gene j (genes int32 [n_sel] with ids in [0, G), repeats allowed; NULL: all genes, n_sel <= G), with c = the count
 * of gene genes[j] in a listed cell:
 *     out[k][0][j] = sum c      out[k][1][j] = the number of listed cells with c != 0      out[k][2][j] = sum fl64(c * w[p])
 * out fp64 [n_seg][3][ld_out]; columns >= n_sel are never written.  w fp64, indexed by LIST POSITION p (not by matrix row), NULL = 1.
 * Arithmetic: a uint16 count adds into 32-bit integer lane sums (exact; a lane sees at most one slab), an fp32 count is widened
 * exactly and added in fp64; the tally is an integer; the weighted term is one fp64 multiply, added in fp64 (never fused).  Lanes
 * hold genes; the waves of a workgroup take a slab's cells round-robin and merge through LDS in wave order; slabs merge in slab
 * order.  No floating-point atomics: two calls agree bit for bit, and because the partial pass always covers all G genes a selected
 * column equals the same column of an all-genes call bit for bit.  A row number outside [0, n_rows) contributes nothing and is
 * never dereferenced; NaN counts are outside the contract.  16-byte loads are used when the matrix base, ld and col_off put every
 * row's first gene on a 16-byte boundary, element loads otherwise (same results).
 * Two launches: spv_count_stats_partial writes one record per (slab, gene) for slabs [slab_first, slab_first + slab_count) into
 * ws fp64 [n_slabs][3][G] (spv_count_stats_ws_bytes(G, n_slabs) bytes, 8-byte aligned; it reads x, G, n_rows, n, pos_off, w, the
 * tables and ws); spv_count_stats_merge adds each segment's records in slab order and applies the gene selection (it reads the
 * tables, ws, genes, n_sel, out, ld_out).  spv_count_stats is both on the whole list (slab_first = pos_off = 0, slab_count =
 * n_slabs).  A caller that holds the listed rows in pieces (a CSR matrix densified chunk by chunk) runs the partial pass once per
 * piece with pos_off = the list position of the piece's first row, then merges once.  Nothing is allocated. */
typedef struct spv_count_stats_args {
  spv_counts x;
  int32_t G, n_rows, n, pos_off;
  const double* w;
  const int32_t* genes;
  const int32_t* slabs;
  const int32_t* seg_slabs;
  int32_t n_sel, n_slabs, n_seg, slab_first, slab_count, pad_;
  double* out; int64_t ld_out;
  void* ws; int64_t ws_bytes;
} spv_count_stats_args;
int spv_count_stats(const spv_count_stats_args* a, void* stream);
int spv_count_stats_partial(const spv_count_stats_args* a, void* stream);
int spv_count_stats_merge(const spv_count_stats_args* a, void* stream);
/* the gene tile T and the slab length S of the partial pass, and its workspace in bytes (0 for a non-positive argument) */
int32_t spv_count_stats_tile(void);
int32_t spv_count_stats_slab(void);
int64_t spv_count_stats_ws_bytes(int32_t G, int32_t n_slabs);

/* total[c] = the sum over all G genes of cell c's counts, fp64 [n_cells], for a dense resident matrix (x->rows is ignored) and for
 * CSR arrays (indptr int64 [n_cells + 1], cols int32 sorted and unique within a row, vals of `dtype`; one wave per row).  uint16
 * counts add as integers (exact); fp32 counts are widened and added in fp64 in ONE fixed order for both forms -- lane t of the cell's
 * wave adds the genes g = t (mod 64) in ascending g, then the 64 lane sums fold by halves -- so the two agree bit for bit (a gene
 * without a stored entry adds an exact zero).  cols is only read for fp32 values. */
int spv_count_totals(const spv_counts* x, int32_t n_cells, int32_t G, double* total, void* stream);
int spv_csr_totals(const int64_t* indptr, const int32_t* cols, const void* vals, int32_t dtype, int32_t n_cells, int32_t G, double* total, void* stream);

/* Exact k-nearest neighbours (spVIPES.latent_neighbors of the user API): for query row i of Q the k rows of C nearest to it, nothing
 * of size n_q x n_c stored.
 * Distance: d(i, j) is the squared Euclidean distance as ONE fp32 chain -- acc = +0; for t = 0 .. D-1 ascending: u = Q[i][t] - C[j][t]
 * (one rounding), acc = fmaf(u, u, acc) (one rounding).  Never the |q|^2 + |c|^2 - 2 q.c form.
 * Order and fill: row i of idx / dist holds the k candidates with the smallest (d, j) in lexicographic order, ascending: equal
 * distances go to the smaller candidate index.  A candidate whose d is not < +inf (overflow, NaN, non-finite input) is never
 * returned, nor is candidate exclude[i] (exclude int32 [n_q] or NULL; a value outside [0, n_c) excludes nothing).  With fewer than k
 * candidates left the remaining slots are idx = -1, dist = +inf.  Columns >= k and rows >= n_q are never written.
 * Independence: the result is a function of (Q, C, D, k, exclude) alone -- the same bit for bit for every n_split (chunks without a
 * candidate included) and for every tiling, two calls agree bit for bit, a query's row does not depend on the other queries of the
 * call, and permuting the candidates permutes idx accordingly wherever distances are distinct.
 * Launches: a partial pass, one workgroup per (tile of spv_knn_tile_q() queries, chunk of the candidates; spv_knn_tile_c() of them
 * in LDS at a time), writes each chunk's sorted list into ws, and a merge pass folds the chunks' lists in the same (d, j) order;
 * n_split == 1 is ONE launch that writes idx / dist itself and needs no workspace.  n_split = 0 stands for
 * spv_knn_splits(n_q, n_c), a pure function of the shapes (no device query) that stays 1 while the query tiles fill the chip.
 * ws: spv_knn_ws_bytes(n_q, k, n_split) bytes with the RESOLVED n_split (0 for n_split <= 1 or a non-positive shape), 8-byte
 * aligned, overwritten by every call.  Nothing is allocated.
 * Rejected ahead of any HIP call with SPV_ERR_ARG: null Q / C / idx / dist; ws null when its size is not 0; D outside
 * [1, SPV_KNN_DMAX]; k outside [1, SPV_KNN_KMAX]; n_split outside [0, SPV_KNN_SPLIT_MAX]; n_q < 1; n_c < 0; ld_q < D; ld_c < D;
 * ld_out < k; n_q * ld_out or n_split * n_q * k beyond 2^31 - 1.  n_c == 0 is valid: every slot is -1 / +inf. */
#define SPV_KNN_DMAX 64
#define SPV_KNN_KMAX 64
#define SPV_KNN_SPLIT_MAX 64
typedef struct spv_knn_args {
  const float* Q; int64_t ld_q; int32_t n_q;      /* queries    fp32 [n_q][ld_q], ld_q >= D */
  const float* C; int64_t ld_c; int32_t n_c;      /* candidates fp32 [n_c][ld_c], ld_c >= D */
  int32_t D;                                      /* 1 .. SPV_KNN_DMAX */
  int32_t k;                                      /* 1 .. SPV_KNN_KMAX */
  const int32_t* exclude;                         /* [n_q] or NULL */
  int32_t n_split;                                /* 0 = spv_knn_splits(n_q, n_c); else 1 .. SPV_KNN_SPLIT_MAX chunks of the candidates */
  int32_t* idx; float* dist; int64_t ld_out;      /* [n_q][ld_out], ld_out >= k */
  void* ws;                                       /* spv_knn_ws_bytes(n_q, k, n_split) bytes */
} spv_knn_args;
int spv_knn(const spv_knn_args* a, void* stream);
int32_t spv_knn_splits(int32_t n_q, int32_t n_c);
int64_t spv_knn_ws_bytes(int32_t n_q, int32_t k, int32_t n_split);
/* queries per workgroup and candidates per LDS tile of the partial pass */
int32_t spv_knn_tile_q(void);
int32_t spv_knn_tile_c(void);

/* spv_knn_paged: the same search for k in [1, SPV_KNN_PAGED_KMAX], on spv_knn's arguments (the one difference is the range of k).
 * Contract: row i of idx / dist holds the k candidates with the smallest (d, j) in lexicographic order, ascending; d is spv_knn's fp32
 * chain, bit for bit; the exclusion, the fill (-1 / +inf) and the non-finite rules are spv_knn's.  The result is a function of
 * (Q, C, D, k, exclude) alone: the same bit for bit for every n_split, independent of the other queries of the call, repeatable bit
 * for bit, and its first min(k, 64) columns are what spv_knn returns for that k, bit for bit.  Columns >= k and rows >= n_q are never
 * written.
 * Mechanism: page p covers the columns [64 p, min(64 p + 64, k)) and is one more run of spv_knn's partial and merge passes (page 0 IS
 * spv_knn's kernels, unchanged).  In page p >= 1 a candidate is offered only if its 64-bit key (the bits of d above j) is GREATER than
 * the key of the query's column 64 p - 1 -- the whole key, not d alone, so a group of equal distances that straddles a page boundary
 * splits by index.  A query whose previous page ended in an empty slot (-1 / +inf: the key after every key that can be made) gets
 * nothing more: its remaining slots are -1 / +inf.  The `after` keys are READ FROM THE OUTPUT ARRAYS: page p reads column 64 p - 1 of
 * idx / dist, which page p - 1 wrote earlier on the same stream, and writes columns >= 64 p only (or the workspace), so nothing a
 * launch reads is written by it.  k <= 64 is one page: 1 or 2 launches; k = 256 is four: 4 or 8.
 * ws: spv_knn_paged_ws_bytes(n_q, k, n_split) = n_split * n_q * min(k, 64) * 8 bytes with the RESOLVED n_split (0 for n_split <= 1 or
 * a non-positive shape), 8-byte aligned, shared by the pages, overwritten by every call: a pure size function, nothing is allocated
 * and no device property is queried.  n_split = 0 stands for spv_knn_splits(n_q, n_c).
 * Rejected ahead of any HIP call with SPV_ERR_ARG, in spv_knn's words: null arguments / Q / C / idx / dist; ws null when its size is
 * not 0, or not 8-byte aligned; D outside [1, SPV_KNN_DMAX]; k outside [1, SPV_KNN_PAGED_KMAX]; n_split outside
 * [0, SPV_KNN_SPLIT_MAX]; n_q < 1; n_c < 0; ld_q < D; ld_c < D; ld_out < k; n_q * ld_out or n_split * n_q * min(k, 64) beyond 2^31 - 1. */
#define SPV_KNN_PAGED_KMAX 256
int spv_knn_paged(const spv_knn_args* a, void* stream);
int64_t spv_knn_paged_ws_bytes(int32_t n_q, int32_t k, int32_t n_split);

/* spv_lisi: the local inverse Simpson index (LISI, Korsunsky et al. 2019) of every row of a neighbour list, for up to
 * SPV_LISI_SETS_MAX label sets on ONE perplexity calibration (spVIPES.latent_lisi / spVIPES.lisi of the user API).
 * Inputs: idx int32 / dist fp32 [n][ld] as spv_knn_paged writes them -- dist the SQUARED distance, ascending, -1 / +inf for an empty
 * slot --, 1 <= k <= SPV_LISI_KMAX; codes int32 [n_sets][n_c], one code per candidate row and label set.  A slot whose dist is not
 * < +inf does not count at all.  A slot whose idx lies outside [0, n_c), or whose code is negative, counts in the calibration (its
 * distance is real) and for NO label.
 * Per row, in fp64: r_j = (double) fl32(sqrt(dist_j)), the correctly rounded fp32 root (the distance latent_neighbors reports);
 * d_j = r_j - r_0 (a shift that leaves the affinities and the entropy unchanged and keeps S >= 1: the published code's underflow case
 * does not arise; a d_j < 0 of a list that does not ascend counts as 0).  Calibration, as compute_simpson of the published code: beta
 * = 1; H = log S + beta T / S with S = sum_j e_j, T = sum_j d_j e_j, e_j = exp(-beta d_j); stop when |H - log(perplexity)| < 1e-5 or
 * after 50 updates; an update doubles (halves) beta while its upper (lower) bound is infinite, else takes the midpoint.  Then
 * p_j = e_j / S, simpson = sum over the labels l of (sum_{j in l} p_j)^2, computed as sum_j p_j s_j with s_j = sum_j' p_j' [code_j' ==
 * code_j] over the slots with a code >= 0, and lisi = 1 / simpson (+inf when no slot has a label).
 * Outputs: lisi fp64 [n_sets][n]; beta fp64 [n]; n_valid int32 [n], the slots that count; converged int32 [n], 0 where the 50 updates
 * ran out.  A row whose slot 0 is not finite (an empty row) gets lisi = NaN, beta = 1, n_valid = 0, converged = 0.
 * Order of addition: one wave per row; lane l holds the slots l, l + 64, l + 128, l + 192.  S, T, simpson and n_valid: the lane adds its
 * slots in ascending slot from +0, then the 64 lane values fold by x += shfl_xor(x, m), m = 32, 16, 8, 4, 2, 1.  s_j: j' = 0 .. k-1 in
 * ascending j' from +0 (a slot that does not match adds +0).  No atomics; two calls agree bit for bit; a row does not depend on the
 * other rows of the call; only equality of codes is asked, so renaming the codes leaves every bit unchanged.
 * Rejected ahead of any HIP call with SPV_ERR_ARG: null arguments / idx / dist / codes / lisi / beta / n_valid / converged; n < 1; k
 * outside [1, SPV_LISI_KMAX]; ld < k; n_c < 0; n_sets outside [1, SPV_LISI_SETS_MAX]; perplexity not a finite number >= 1. */
#define SPV_LISI_KMAX 256
#define SPV_LISI_SETS_MAX 8
typedef struct spv_lisi_args {
  const int32_t* idx; const float* dist; int64_t ld;   /* [n][ld], ld >= k */
  int32_t n; int32_t k;                           /* rows; 1 .. SPV_LISI_KMAX slots per row */
  const int32_t* codes; int32_t n_c; int32_t n_sets;   /* [n_sets][n_c]; 1 .. SPV_LISI_SETS_MAX */
  double perplexity;                              /* finite, >= 1 */
  double* lisi;                                   /* [n_sets][n] */
  double* beta; int32_t* n_valid; int32_t* converged;   /* [n] */
} spv_lisi_args;
int spv_lisi(const spv_lisi_args* a, void* stream);

/* Entropic optimal transport between two point clouds (spVIPES.compute_transport_plan of the user API): the two reductions a
 * log-domain Sinkhorn iteration and a sparse plan need, over all (query, candidate) pairs, nothing of size n_q x n_c stored.
 * Per pair: c(i, j) = the distance of spv_knn above, the same bits (so c(x, y) and c(y, x) are the same bits: u and -u square
 * alike), and t(i, j) = fmaf(-c(i, j), inv_eps, h[j]), ONE rounding.  h fp32 [n_c]: the caller's psi_j + log b_j.
 * spv_ot_softmin: L[i] = log sum_j exp(t(i, j)), fp32 [n_q].  Per query a running (m, sum) pair over its chunk in ascending j, one exp
 * per candidate -- e = exp(-|t - m|); t > m: sum = fmaf(sum, e, 1), m = t; else sum += e -- and L = m + log(sum).  A t that is not finite
 * contributes nothing: h[j] = -inf marks a candidate of zero mass, an overflowing cost gives t = -inf, a NaN is skipped.  A query
 * without a contributing candidate (n_c == 0 included) gets L = -inf.
 * spv_ot_topk: row i of idx / val holds the k candidates with the largest t(i, j), in descending t, equal t to the smaller j; a t
 * that is not finite is never selected.  val = exp(t(i, j) + r[i]) (r fp32 [n_q]: phi_i + log a_i), i.e. the plan entry P_ij;
 * mass[i] = the fp32 sum of row i's val, added in list order from +0.  With fewer than k selectable candidates the remaining slots
 * are idx = -1, val = 0.  Columns >= k and rows >= n_q are never written.  idx is exact: a function of the t bits alone, the same for
 * every n_split and tiling, and a query's row does not depend on the other queries of the call.
 * Launches: as spv_knn -- a partial pass of (tiles of spv_ot_tile_q() queries) x (n_split chunks of the candidates,
 * spv_ot_tile_c() of them in LDS at a time) workgroups, and for n_split > 1 a merge pass, one lane per query, that folds the chunks'
 * (m, sum) pairs / sorted lists from ws IN CHUNK ORDER.  No floating-point atomics: for fixed shapes and n_split two calls agree bit
 * for bit.  L under DIFFERENT n_split agrees within its rounding bound only (a sum's grouping changes its rounding), not bit for bit.
 * n_split = 0 stands for spv_ot_splits(n_q, n_c), a pure function of the shapes.
 * ws: spv_ot_ws_bytes(n_q, k, n_split) bytes with the RESOLVED n_split; k = 0 asks for spv_ot_softmin's size.  8-byte aligned,
 * overwritten by every call.  Nothing is allocated.
 * Rejected ahead of any HIP call with SPV_ERR_ARG, both entry points: null arguments / Q / C / h; ws null when its size is not 0 or
 * not 8-byte aligned; D outside [1, SPV_OT_DMAX]; n_split outside [0, SPV_OT_SPLIT_MAX]; n_q < 1; n_c < 0; ld_q < D; ld_c < D;
 * inv_eps not a positive finite number; n_split * n_q (softmin) or n_split * n_q * k (topk) beyond 2^31 - 1.  spv_ot_softmin: null L.
 * spv_ot_topk: null r / idx / val / mass; k outside [1, SPV_OT_KMAX]; ld_out < k; n_q * ld_out beyond 2^31 - 1. */
#define SPV_OT_DMAX 64
#define SPV_OT_KMAX 64
#define SPV_OT_SPLIT_MAX 64
typedef struct spv_ot_args {
  const float* Q; int64_t ld_q; int32_t n_q;      /* queries    fp32 [n_q][ld_q], ld_q >= D */
  const float* C; int64_t ld_c; int32_t n_c;      /* candidates fp32 [n_c][ld_c], ld_c >= D */
  int32_t D;                                      /* 1 .. SPV_OT_DMAX */
  int32_t k;                                      /* spv_ot_topk: 1 .. SPV_OT_KMAX; spv_ot_softmin ignores it */
  const float* h;                                 /* [n_c] */
  const float* r;                                 /* [n_q], spv_ot_topk */
  float inv_eps;                                  /* s = 1 / epsilon, > 0 */
  int32_t n_split;                                /* 0 = spv_ot_splits(n_q, n_c); else 1 .. SPV_OT_SPLIT_MAX chunks of the candidates */
  float* L;                                       /* [n_q], spv_ot_softmin */
  int32_t* idx; float* val; int64_t ld_out;       /* [n_q][ld_out], ld_out >= k, spv_ot_topk */
  float* mass;                                    /* [n_q], spv_ot_topk */
  void* ws;                                       /* spv_ot_ws_bytes(n_q, k or 0, n_split) bytes */
} spv_ot_args;
int spv_ot_softmin(const spv_ot_args* a, void* stream);
int spv_ot_topk(const spv_ot_args* a, void* stream);
int32_t spv_ot_splits(int32_t n_q, int32_t n_c);
int64_t spv_ot_ws_bytes(int32_t n_q, int32_t k, int32_t n_split);
/* queries per workgroup and candidates per LDS tile of the partial passes */
int32_t spv_ot_tile_q(void);
int32_t spv_ot_tile_c(void);

/* The plan's log mass between every query and every SEGMENT of the candidates (spVIPES.match_transport_clusters of the user API):
 * the candidates come ARRANGED BY SEGMENT, and for query row i and segment s
 *   L[s][i] = log sum over j in [seg_ptr[s], seg_ptr[s + 1]) of exp(t(i, j)),   t(i, j) = fmaf(-c(i, j), inv_eps, h[j])
 * with spv_ot_softmin's c and t, the same bits; nothing of size n_q x n_c stored.  With h = psi + log b and r_i = phi_i + log a_i of a
 * Sinkhorn result, exp(L[s][i] + r_i) is the mass the untruncated plan puts between cell i and the cells of segment s.
 * Per lane ONE running (m, sum) pair, updated as spv_ot_softmin's; at a segment's end (the same candidate for every lane) it is
 * written and re-initialised.  A t that is not finite contributes nothing; a segment without a contributing candidate -- an empty
 * one, n_c == 0 -- gives -inf.
 * seg_ptr: int32 [n_seg + 1] ON THE DEVICE, ascending, seg_ptr[0] = 0, seg_ptr[n_seg] = n_c; empty segments are allowed.  It cannot
 * be checked from the host: any other content gives unspecified values, never an access outside seg_ptr, L or ws.
 * Layout of L: SEGMENT-MAJOR, fp32 [n_seg][ld_l] with ld_l >= n_q -- L[s * ld_l + i].  Columns >= n_q are never written.
 * Launches: a partial pass of (tiles of spv_ot_tile_q() queries) x (n_split chunks of the candidates) workgroups; n_split == 1 is ONE
 * launch that writes L itself; for n_split > 1 every (tile, chunk) writes all n_seg states to ws and a merge pass, one lane per
 * (query, segment), folds them IN CHUNK ORDER.  No floating-point atomics: for fixed shapes and n_split two calls agree bit for bit,
 * and a query's values do not depend on the other queries of the call.  Different n_split agree within spv_ot_softmin's rounding
 * bound, not bit for bit.  The chunks of a given n_split are spv_ot_softmin's: with n_seg == 1 and the same EXPLICIT n_split, L[0]
 * equals spv_ot_softmin's L bit for bit.  n_split = 0 stands for spv_ot_segment_splits(n_q, n_c), a pure function of the shapes
 * (more chunks than spv_ot_splits: a chunk's state is small).
 * ws: spv_ot_segment_ws_bytes(n_q, n_seg, n_split) bytes with the RESOLVED n_split (0 for n_split <= 1 or a non-positive shape;
 * 64-bit arithmetic), 8-byte aligned, overwritten by every call.  Nothing is allocated.
 * Rejected ahead of any HIP call with SPV_ERR_ARG: null arguments / Q / C / h / seg_ptr / L; ws null when its size is not 0, or not
 * 8-byte aligned; D outside [1, SPV_OT_DMAX]; n_split outside [0, SPV_OT_SPLIT_MAX]; n_q < 1; n_c < 0; ld_q < D; ld_c < D; inv_eps
 * not a positive finite number; n_seg outside [1, SPV_OT_SEG_MAX]; ld_l < n_q; n_seg * ld_l or n_split * n_seg * n_q beyond 2^31 - 1. */
#define SPV_OT_SEG_MAX 256
typedef struct spv_ot_seg_args {
  const float* Q; int64_t ld_q; int32_t n_q;      /* queries    fp32 [n_q][ld_q], ld_q >= D */
  const float* C; int64_t ld_c; int32_t n_c;      /* candidates fp32 [n_c][ld_c], ld_c >= D, arranged by segment */
  int32_t D;                                      /* 1 .. SPV_OT_DMAX */
  const float* h;                                 /* [n_c] */
  float inv_eps;                                  /* s = 1 / epsilon, > 0 */
  const int32_t* seg_ptr; int32_t n_seg;          /* [n_seg + 1] on the device; 1 .. SPV_OT_SEG_MAX segments */
  int32_t n_split;                                /* 0 = spv_ot_segment_splits(n_q, n_c); else 1 .. SPV_OT_SPLIT_MAX chunks of the candidates */
  float* L; int64_t ld_l;                         /* [n_seg][ld_l], ld_l >= n_q */
  void* ws;                                       /* spv_ot_segment_ws_bytes(n_q, n_seg, n_split) bytes */
} spv_ot_seg_args;
int spv_ot_segment_lse(const spv_ot_seg_args* a, void* stream);
int32_t spv_ot_segment_splits(int32_t n_q, int32_t n_c);
int64_t spv_ot_segment_ws_bytes(int32_t n_q, int32_t n_seg, int32_t n_split);

/* Barycentric projection through the untruncated plan (spVIPES.transport_project of the user API): for query row i the
 * plan-weighted mean of the candidates' value rows,
 *   out[v][i] = sum_j exp(t(i, j)) V[j][v] / sum_j exp(t(i, j)),   t(i, j) = fmaf(-c(i, j), inv_eps, h[j]),   L[i] = log sum_j exp(t(i, j))
 * with spv_ot_softmin's c and t, the same bits; nothing of size n_q x n_c stored.  With h = psi + log b of a Sinkhorn result the
 * weights are row i of the plan up to the row's own factor, which the quotient drops; exp(L[i] + phi_i + log a_i) is the row's mass.
 * Per lane a running (m, sum) pair, updated as spv_ot_softmin's, and one accumulator per value column.  Per candidate with a finite
 * t: d = t - m, e = exp(-|d|), and ONE fma per column: acc = fmaf(acc, e, V[j][v]) for d > 0, acc = fmaf(e, V[j][v], acc) otherwise.
 * A t that is not finite contributes nothing and its value row enters no sum, whatever it holds.  out = acc / sum, the correctly
 * rounded quotient.  A query without a contributing candidate (n_c == 0 included) gets L = -inf and NaN in every column.
 * A column of ones repeats the sum's operations and comes back as exactly 1.0f.
 * V: fp32 [n_c][ld_v], ld_v >= n_v.  Layout of out: VALUE-MAJOR, fp32 [n_v][ld_out] with ld_out >= n_q -- out[v * ld_out + i].  L: fp32
 * [n_q], may be NULL.  Rows >= n_q, columns >= n_v and everything beyond the workspace's bytes are never written.
 * Launches: a partial pass of (tiles of spv_ot_tile_q() queries) x (n_split chunks of the candidates) x (blocks of
 * spv_ot_project_block(D) value columns) workgroups, every column block rescanning the distances; n_split == 1 is ONE launch that
 * writes out and L; for n_split > 1 every workgroup writes (m, sum, its accumulators) to ws and a merge pass, one lane per (query,
 * column), folds the chunks IN CHUNK ORDER: a later chunk with the larger m gives acc = fmaf(acc, e, its acc), otherwise (if its sum is
 * positive) acc = fmaf(its acc, e, acc), next to spv_ot_softmin's merge of (m, sum).  No floating-point atomics: for fixed shapes and
 * n_split two calls agree bit for bit; a query's row does not depend on the other queries of the call, and a column's values not on
 * which other columns the call holds.  Different n_split agree within rounding.  The chunks of a given n_split are spv_ot_softmin's:
 * at the same EXPLICIT n_split L equals spv_ot_softmin's L bit for bit.  n_split = 0 stands for spv_ot_project_splits(n_q, n_c, n_v), a
 * pure function of the shapes.
 * ws: spv_ot_project_ws_bytes(n_q, n_v, n_split) bytes with the RESOLVED n_split (0 for n_split <= 1 or a non-positive shape; 64-bit
 * arithmetic; enough for every D), 8-byte aligned, overwritten by every call.  Nothing is allocated.
 * Rejected ahead of any HIP call with SPV_ERR_ARG: null arguments / Q / C / h / out; V null while n_c > 0; ws null when its size is not
 * 0, or not 8-byte aligned; D outside [1, SPV_OT_DMAX]; n_v outside [1, SPV_OT_VAL_MAX]; n_split outside [0, SPV_OT_SPLIT_MAX]; n_q < 1;
 * n_c < 0; ld_q < D; ld_c < D; ld_v < n_v; ld_out < n_q; inv_eps not a positive finite number; n_v * ld_out or the workspace's word
 * count beyond 2^31 - 1. */
#define SPV_OT_VAL_MAX 256
typedef struct spv_ot_proj_args {
  const float* Q; int64_t ld_q; int32_t n_q;      /* queries    fp32 [n_q][ld_q], ld_q >= D */
  const float* C; int64_t ld_c; int32_t n_c;      /* candidates fp32 [n_c][ld_c], ld_c >= D */
  int32_t D;                                      /* 1 .. SPV_OT_DMAX */
  const float* h;                                 /* [n_c] */
  float inv_eps;                                  /* s = 1 / epsilon, > 0 */
  const float* V; int64_t ld_v; int32_t n_v;      /* values     fp32 [n_c][ld_v], ld_v >= n_v; 1 .. SPV_OT_VAL_MAX columns */
  int32_t n_split;                                /* 0 = spv_ot_project_splits(n_q, n_c, n_v); else 1 .. SPV_OT_SPLIT_MAX chunks of the candidates */
  float* out; int64_t ld_out;                     /* [n_v][ld_out], ld_out >= n_q */
  float* L;                                       /* [n_q] or NULL */
  void* ws;                                       /* spv_ot_project_ws_bytes(n_q, n_v, n_split) bytes */
} spv_ot_proj_args;
int spv_ot_project(const spv_ot_proj_args* a, void* stream);
int32_t spv_ot_project_splits(int32_t n_q, int32_t n_c, int32_t n_v);
int64_t spv_ot_project_ws_bytes(int32_t n_q, int32_t n_v, int32_t n_split);
/* value columns per column block of the kernel form that serves D columns of Q / C; 0 for a D outside [1, SPV_OT_DMAX] */
int32_t spv_ot_project_block(int32_t D);

/* Segmented distance sums (spVIPES.latent_silhouette / integration_scores of the user API): for query row i of Q and every segment s
 * of the candidates C, which come ARRANGED BY SEGMENT, the fp64 sum of the Euclidean distances to the segment's rows; nothing of size
 * n_q x n_c stored.
 *   S[s][i] = sum over j in [seg_ptr[s], seg_ptr[s + 1]) of (double) d(i, j),   d(i, j) = fl32(sqrt(d2(i, j)))
 * d2 is the distance of spv_knn above, the same bits; the root is the correctly rounded fp32 one.  A query that is also a candidate
 * adds d = +0 for itself.  An empty segment gives +0.  A non-finite candidate row makes its segment's sums NaN / inf, a non-finite
 * query row all of its own sums, nothing else.
 * seg_ptr: int32 [n_seg + 1] ON THE DEVICE, ascending, seg_ptr[0] = 0, seg_ptr[n_seg] = n_c; empty segments are allowed.  It cannot
 * be checked from the host: any other content gives unspecified sums, never an access outside seg_ptr, S or ws.
 * Layout of S: SEGMENT-MAJOR, fp64 [n_seg][ld_s] with ld_s >= n_q -- S[s * ld_s + i] -- so that the lanes of a workgroup, one query
 * each, write consecutive doubles when a segment ends.  Columns >= n_q are never written.
 * Order of addition: ascending j within a chunk of the candidates, ascending chunk across chunks, from +0; no floating-point atomics.
 * For fixed shapes and n_split two calls agree bit for bit, and a query's sums do not depend on the other queries of the call.  Under
 * DIFFERENT n_split the sums may differ in the last bits of fp64, except where every partial sum is exact.
 * Launches: as spv_knn -- a partial pass of (tiles of spv_knn_tile_q() queries) x (n_split chunks of the candidates) workgroups, and
 * for n_split > 1 a merge pass over the workspace; n_split == 1 is ONE launch that writes S itself.  n_split = 0 stands for
 * spv_silhouette_splits(n_q, n_c), a pure function of the shapes.
 * ws: spv_silhouette_ws_bytes(n_q, n_seg, n_split) bytes with the RESOLVED n_split (0 for n_split <= 1 or a non-positive shape;
 * 64-bit arithmetic), 8-byte aligned, overwritten by every call.  Nothing is allocated.
 * Rejected ahead of any HIP call with SPV_ERR_ARG: null arguments / Q / C / seg_ptr / S; ws null when its size is not 0, or not
 * 8-byte aligned; D outside [1, SPV_KNN_DMAX]; n_seg outside [1, SPV_SILHOUETTE_SEG_MAX]; n_split outside [0, SPV_KNN_SPLIT_MAX];
 * n_q < 1; n_c < 0; ld_q < D; ld_c < D; ld_s < n_q.  n_c == 0 is valid: every sum is +0. */
#define SPV_SILHOUETTE_SEG_MAX 256
typedef struct spv_silhouette_args {
  const float* Q; int64_t ld_q; int32_t n_q;      /* queries    fp32 [n_q][ld_q], ld_q >= D */
  const float* C; int64_t ld_c; int32_t n_c;      /* candidates fp32 [n_c][ld_c], ld_c >= D, arranged by segment */
  int32_t D;                                      /* 1 .. SPV_KNN_DMAX */
  const int32_t* seg_ptr; int32_t n_seg;          /* [n_seg + 1] on the device; 1 .. SPV_SILHOUETTE_SEG_MAX segments */
  int32_t n_split;                                /* 0 = spv_silhouette_splits(n_q, n_c); else 1 .. SPV_KNN_SPLIT_MAX chunks of the candidates */
  double* S; int64_t ld_s;                        /* [n_seg][ld_s], ld_s >= n_q */
  void* ws;                                       /* spv_silhouette_ws_bytes(n_q, n_seg, n_split) bytes */
} spv_silhouette_args;
int spv_silhouette_sums(const spv_silhouette_args* a, void* stream);
int32_t spv_silhouette_splits(int32_t n_q, int32_t n_c);
int64_t spv_silhouette_ws_bytes(int32_t n_q, int32_t n_seg, int32_t n_split);

/* The fp64 Gram of an fp32 block (spVIPES.get_feature_correlation_matrix of the user API): over the counted rows r of x
 *   sums[j] += sum_r (double) x[r][j]          gram[i][j] += sum_r (double) x[r][i] * (double) x[r][j],   i, j < n, BOTH triangles
 * Every x is widened to fp64 first, so every product is exact; the sums run in v_mfma_f64_16x16x4_f64 accumulators with the rows fed
 * in ascending order, and the tables carry summation error only: every element lies within gamma_m (|start| + sum |x_i x_j|) of the
 * exact value, gamma_m = m u / (1 - m u), u = 2^-53, m = n_use + slabs + 1.
 * rows: NULL -- rows 0 .. n_rows - 1 count and n_use is ignored -- or n_use strictly ascending row numbers in [0, n_rows) ON THE
 * DEVICE.  They cannot be checked from the host: a number outside the block is clamped into it (a wrong row is added, nothing outside
 * x is read), a repeated one is counted as often as it is listed.  Rows that are not listed and columns >= n of x are never read and
 * may hold NaN.
 * Both tables ACCUMULATE: zero them once, then one pair collects a whole walk.  gram[i][j] and its mirror gram[j][i] take the same
 * addend -- the upper triangle is computed, diagonal tiles included, and stored twice -- so a table that is symmetric in bits stays so.
 * Columns >= n of gram's rows are never touched.
 * No floating-point atomics and every order fixed: one workgroup owns one 64 x 64 tile of the upper triangle and one slab of the counted
 * rows; with spv_gram_slabs(n, n_use) > 1 the partial tiles go to ws and a merge launch of the same call adds them in ascending slab
 * order from +0, then onto the tables.  Each table element has one writer.  The slab count is a pure function of (n, n_use): two calls
 * agree bit for bit.  One slab (always at n >= 2048) is ONE launch and needs no workspace.
 * ws: spv_gram_ws_bytes(n, n_use) bytes (at most 32 537 600, at n = 1984; 0 for one slab), 8-byte aligned, overwritten by every call;
 * nothing beyond those bytes is touched.  Nothing is allocated.
 * n_use == 0, or rows == NULL with n_rows == 0: success, nothing changes.
 * Rejected ahead of any HIP call with SPV_ERR_ARG: null arguments / x / sums / gram; n outside [1, SPV_GRAM_MAX_N]; n_rows < 0;
 * n_use < 0 (with rows); ld_x < n; ld_gram < n; x not 4-byte aligned; sums, gram or ws not 8-byte aligned; ws null or ws_bytes short
 * when the shape needs a workspace. */
#define SPV_GRAM_MAX_N 4096
typedef struct spv_gram_args {
  const float* x; int64_t ld_x; int32_t n_rows;   /* fp32 block [n_rows][ld_x >= n], unit column stride */
  const int32_t* rows; int32_t n_use;             /* NULL, or n_use strictly ascending row numbers in [0, n_rows) on the device */
  int32_t n;                                      /* columns, 1 .. SPV_GRAM_MAX_N */
  double* sums;                                   /* [n] */
  double* gram; int64_t ld_gram;                  /* [n][ld_gram >= n] */
  void* ws; uint64_t ws_bytes;                    /* spv_gram_ws_bytes(n, n_use) bytes or more */
} spv_gram_args;
int spv_gram_f64(const spv_gram_args* a, void* stream);
int32_t spv_gram_slabs(int32_t n, int32_t n_use);   /* row slabs used for this shape; a function of (n, n_use) only */
uint64_t spv_gram_ws_bytes(int32_t n, int32_t n_use);

/* Rank sums of the OBSERVED counts (spVIPES.rank_genes_groups of the user API: the Wilcoxon / Mann-Whitney rank-sum test of every
 * label against the rest): a segmented column sort with tie runs.  The kernels work on a LIST of n positions, 1 <= n <= SPV_RANK_MAX_N.
 * Position p names the cell x.rows[p - pos_off] (x.rows == NULL: cell p - pos_off) of a dense matrix that holds the positions
 * [pos_off, pos_off + n_piece) -- spv_count_stats' addressing -- and carries a segment code seg[p] (int32 [n]; n_seg <=
 * SPV_RANK_MAX_SEG) and an optional weight w[p] (fp32 [n], indexed by LIST POSITION, NULL = none).  A call covers a slab of n_sel <=
 * spv_rank_gene_slab() selected genes (genes int32 [n_sel] with ids in [0, G), repeats allowed; NULL: genes 0 .. n_sel - 1, n_sel <= G).
 * Key: for selected gene j the key of position p is the fp32 value key = (float) c * w[p], ONE fp32 multiply that is never contracted
 * with anything ((float) c without w), c = the count of gene genes[j] in the cell: uint16, or a non-negative finite fp32.  Negative or
 * NaN counts and negative weights are outside the contract.  Keys are non-negative: their bit pattern orders them; every zero key
 * (also 0 * w and c * 0) is the one pattern 0.
 * Outputs, per selected gene j, WRITTEN (not accumulated); columns >= n_sel of rank2 are never touched:
 *     rank2[k][j] = the sum over the positions p of segment k of L + U + 1      int64 [n_seg][ld_rank2 >= n_sel]
 *     ties[j]     = the sum over the runs of equal keys of t^3 - t              int64 [n_sel], at most 2^60 at n = 2^20
 * with L = the number of list positions whose key in gene j is smaller than p's and U = the number whose key is smaller or equal, so
 * that L + U + 1 is twice p's average rank.  Every sum is an integer sum collected with 64-bit integer atomics in LDS; there is no
 * floating-point atomic; two calls agree bit for bit and the order inside a run of equal keys is free.
 * A segment code outside [0, n_seg) is ranked with the others (it counts in their L and U) but adds to no sum and never indexes a
 * table.  A row number outside [0, n_rows) and a gene id outside [0, G) read as a zero count and are never dereferenced.
 * Two entry points over one workspace of spv_rank_ws_bytes(n, n_sel) = 8192 + 16 n n_sel bytes, 8-byte aligned:
 *   spv_rank_stage  reads the piece [pos_off, pos_off + n_piece) of the list from x (a dense resident matrix, or a CSR chunk densified
 *     by spv_csr_gather) and appends the piece's NON-ZERO keys, with their segment codes, to the genes' columns in the workspace (gene-major,
 *     through an LDS transpose and one integer atomic cursor per gene; all zero keys form one run at the bottom and are accounted for from
 *     counts: the positions of each segment are tallied here as well).  reset != 0 empties the columns first: set it for the first piece
 *     of a list and only there.  A caller with the rows in pieces runs it once per piece (as spv_count_stats_partial); every position must
 *     be staged exactly once (a piece staged twice is counted twice; nothing is written outside the workspace).  It reads x, G, n_rows,
 *     n_piece, pos_off, n, n_seg, n_sel, reset, seg, w, genes, ws.
 *   spv_rank_sums   sorts every staged column (one workgroup per gene: in LDS up to spv_rank_lds_capacity() non-zero keys, else by
 *     radix passes of spv_rank_sort_tile() entries through the workspace's second half), walks the tie runs and writes rank2 and ties.
 *     It reads n, n_seg, n_sel, rank2, ld_rank2, ties, ws; the staged columns are consumed (their order changes).
 * Nothing is allocated.  Rejected ahead of any HIP call with SPV_ERR_ARG, both entry points: null arguments; n outside [1, SPV_RANK_MAX_N];
 * n_seg outside [1, SPV_RANK_MAX_SEG]; n_sel outside [1, spv_rank_gene_slab()]; ws null, not 8-byte aligned, or ws_bytes short.
 * spv_rank_stage: null x.X / seg; unknown dtype; G or n_rows < 1; n_piece < 1, pos_off < 0 or pos_off + n_piece > n; n_piece > n_rows
 * without a row list; ld < col_off + G; n_sel > G without a gene list.  spv_rank_sums: null rank2 / ties; ld_rank2 < n_sel; rank2 or
 * ties not 8-byte aligned. */
#define SPV_RANK_MAX_N (1 << 20)
#define SPV_RANK_MAX_SEG 1024
typedef struct spv_rank_args {
  spv_counts x;                            /* stage: the matrix that holds the piece */
  int32_t G, n_rows, n_piece, pos_off;     /* stage */
  int32_t n, n_seg, n_sel, reset;          /* the list, the segments, the gene slab; reset: stage only */
  const int32_t* seg;                      /* [n] */
  const float* w;                          /* [n] or NULL */
  const int32_t* genes;                    /* [n_sel] or NULL */
  int64_t* rank2; int64_t ld_rank2;        /* sums: [n_seg][ld_rank2 >= n_sel] */
  int64_t* ties;                           /* sums: [n_sel] */
  void* ws; int64_t ws_bytes;              /* spv_rank_ws_bytes(n, n_sel) bytes or more */
} spv_rank_args;
int spv_rank_stage(const spv_rank_args* a, void* stream);
int spv_rank_sums(const spv_rank_args* a, void* stream);
/* pure shape functions: the most genes per call; the workspace in bytes (8-byte multiple; 0 for a non-positive or out-of-range argument);
 * the switch point between the LDS-resident sort and the radix passes (non-zero keys of one gene); the stage's tile of list positions;
 * the entries one radix tile moves */
int32_t spv_rank_gene_slab(void);
int64_t spv_rank_ws_bytes(int32_t n, int32_t n_sel);
int32_t spv_rank_lds_capacity(void);
int32_t spv_rank_stage_tile(void);
int32_t spv_rank_sort_tile(void);

/* The rank transform on the same column sort (rank_ops.rank_transform; spVIPES.get_feature_spearman_matrix / count_spearman_matrix of
 * the user API): every list position gets its rank back, as the fp32 block spv_gram_f64 reads.  The list, the addressing of x, the
 * weights, the gene slab and the key (ONE fp32 multiply, zero keys all the pattern 0) are spv_rank_stage's; there are no segments.
 * Output, WRITTEN for every list position p < n and slab gene j < n_sel; columns >= n_sel of out are never touched:
 *     out[p * ld_out + j] = (float)(L + U - n) = (float)(2 * average rank of p among the n keys of gene j - (n + 1))
 * with L = the list positions whose key is smaller than p's and U = those whose key is smaller or equal.  An integer in
 * [-(n - 1), n - 1], exact in fp32; every column sums to exactly 0 and its squares to exactly (n^3 - n - ties[j]) / 3.  All zero keys
 * form one run at the bottom and are never stored or sorted: a zero key gets n_zero - n, a stored key of the run [s, e) of its sorted
 * column 2 n_zero + s + e - n.
 *     ties[j]    = the sum over the runs of equal keys, the zero run included, of t^3 - t (spv_rank_sums' ties)   int64 [n_sel] or NULL
 *     nonzero[j] = the stored (non-zero) keys of gene j                                                            int32 [n_sel] or NULL
 * Every output element has one writer; the walk and the store use no atomic of any kind (the shared sort keeps its integer LDS
 * histogram, the stage its integer cursor; no floating-point atomic anywhere): two calls agree bit for bit.
 * Two entry points over one workspace of spv_rank_values_ws_bytes(n, n_sel) = spv_rank_ws_bytes(n, n_sel) + 4 n n_sel bytes, rounded up
 * to a multiple of 8, 8-byte aligned:
 *   spv_rank_values_stage  spv_rank_stage with the list position in the place of the segment code: appends the NON-ZERO keys of the
 *     piece [pos_off, pos_off + n_piece) to the genes' columns.  reset != 0 empties the columns first (the first piece of a list, and
 *     only there); every position must be staged exactly once.  It reads x, G, n_rows, n_piece, pos_off, n, n_sel, reset, w, genes, ws.
 *   spv_rank_values        sorts every staged column (spv_rank_sums' two routes), fills the gene's fp32 column in the workspace with the
 *     zero run's value, scatters the stored entries' values by position, and a second launch moves 64 x 64 tiles into the row-major out.
 *     It reads n, n_sel, out, ld_out, ties, nonzero, ws; the staged columns are consumed.  out may be the staged matrix itself: the
 *     call reads the workspace only.
 * A position word at or above n is never used as an address; a gene's stored keys are cut to n; a row number outside [0, n_rows) and a
 * gene id outside [0, G) read as a zero key and are never dereferenced.
 * Nothing is allocated.  Rejected ahead of any HIP call with SPV_ERR_ARG, both entry points: null arguments; n outside [1, SPV_RANK_MAX_N];
 * n_sel outside [1, spv_rank_gene_slab()]; ws null, not 8-byte aligned, or ws_bytes short.  spv_rank_values_stage: null x.X; unknown
 * dtype; G or n_rows < 1; n_piece < 1, pos_off < 0 or pos_off + n_piece > n; n_piece > n_rows without a row list; ld < col_off + G;
 * n_sel > G without a gene list.  spv_rank_values: null out; out or nonzero not 4-byte aligned; ties not 8-byte aligned; ld_out < n_sel. */
typedef struct spv_rank_values_args {
  spv_counts x;                            /* stage: the matrix that holds the piece */
  int32_t G, n_rows, n_piece, pos_off;     /* stage */
  int32_t n, n_sel, reset;                 /* the list, the gene slab; reset: stage only */
  const float* w;                          /* [n] or NULL */
  const int32_t* genes;                    /* [n_sel] or NULL */
  float* out; int64_t ld_out;              /* values: [n][ld_out >= n_sel], row-major */
  int64_t* ties;                           /* values: [n_sel] or NULL */
  int32_t* nonzero;                        /* values: [n_sel] or NULL */
  void* ws; int64_t ws_bytes;              /* spv_rank_values_ws_bytes(n, n_sel) bytes or more */
} spv_rank_values_args;
int spv_rank_values_stage(const spv_rank_values_args* a, void* stream);
int spv_rank_values(const spv_rank_values_args* a, void* stream);
/* the workspace in bytes (8-byte multiple; 0 for a non-positive or out-of-range argument, like spv_rank_ws_bytes) */
int64_t spv_rank_values_ws_bytes(int32_t n, int32_t n_sel);

/* PCA of the log-normalised OBSERVED counts (pca_ops.block_lanczos; spVIPES.count_pca / spVIPES.pca of the user API): the operand
 * stage and the two skinny products of a block Krylov step against a matrix X [n][G] that is never stored.  The list, the piece and
 * the addressing of x are spv_rank_stage's: position p of a list of n names the cell x.rows[p - pos_off] (x.rows == NULL: cell
 * p - pos_off) of a dense matrix that holds the positions [pos_off, pos_off + n_piece); w is an optional fp32 weight per LIST POSITION.
 * The operand, the same device function in all three kernels, for the count c (uint16, or a non-negative finite fp32) of gene j:
 *     u = (float) c * w[p]          ONE fp32 multiply, never contracted (spv_rank_stage's key; (float) c without w)
 *     a = pca_log1p(u)              one fixed sequence of fp32 operations (csrc/spv_pca.h), a == 0 exactly for u == 0
 *     x(p, j) = (a - mu[j]) * scale[j]     an fp32 subtract, then an fp32 multiply, not fused; mu == NULL reads as 0, scale == NULL as 1
 * A gene with scale[j] == 0 contributes exactly 0: a gene selection is a scale vector; every kernel walks all G genes and gathers no
 * column.  A row number outside [0, n_rows) reads as a zero count and is never dereferenced.  l is 16, 32, 48 or 64.
 *   spv_pca_stage    WRITES block[(p - pos_off) * ld_block + j] = x(p, j), fp32 [n_piece][ld_block >= G]; columns >= G are never touched.
 *     It reads x, G, n_rows, n_piece, pos_off, n, w, mu, scale, block, ld_block.
 *   spv_pca_project  WRITES Y[p * ld_y + t] = sum_j x(p, j) V[j * ld_v + t] for the piece's positions and t < l.  V fp32 [G][ld_v >= l],
 *     Y fp32 [n][ld_y >= l].  One workgroup owns spv_pca_cell_tile() positions and walks the genes in ascending order into
 *     v_mfma_f32_32x32x2_f32 accumulators: every product is exact, the sum of a row is ONE fp32 chain over the genes 0 .. G - 1.  A
 *     row's result depends on that row alone: not on the piece, not on the other rows, not on dense or CSR storage.
 *   spv_pca_back     ADDS sum_p x(p, j) Y[p * ld_y + t] over the piece's positions onto Z[j * ld_z + t], fp64 [G][ld_z >= l].  The list
 *     is cut into slabs at ABSOLUTE positions, multiples of spv_pca_slab(); pos_off must be one.  One workgroup per (64 genes, slab)
 *     sums its slab in ascending position order on the same MFMA and stores an fp32 partial tile to ws; a merge launch of the same
 *     call adds the piece's slabs onto Z in ascending slab order, one fp64 addition per slab.  No floating-point atomics, every element
 *     one writer, every order fixed: a list passed in one piece or in slab-aligned pieces (in list order) gives the same bits, two
 *     calls agree bit for bit, and the calls of several groups collect in one Z.
 *     ws: spv_pca_ws_bytes(G, n_piece, l) = 4 * ceil(n_piece / slab) * round_up(G, 64) * l bytes, 8-byte aligned, overwritten.
 * Nothing is allocated.  Rejected ahead of any HIP call with SPV_ERR_ARG, all three: null arguments / x.X; unknown dtype; G, n_rows, n
 * or n_piece < 1; pos_off < 0 or pos_off + n_piece > n; n_piece > n_rows without a row list; ld < col_off + G.  stage: null block;
 * ld_block < G.  project and back: l not 16, 32, 48 or 64; null Y; ld_y < l.  project: null V; ld_v < l.  back: pos_off off a slab
 * bound; null Z; Z not 8-byte aligned; ld_z < l; ws null, not 8-byte aligned, or ws_bytes short. */
typedef struct spv_pca_args {
  spv_counts x;                            /* the matrix that holds the piece */
  int32_t G, n_rows, n_piece, pos_off;
  int32_t n, l;                            /* the list; the columns of V / Y / Z */
  const float* w;                          /* [n] or NULL */
  const float* mu;                         /* [G] or NULL */
  const float* scale;                      /* [G] or NULL */
  float* block; int64_t ld_block;          /* stage: [n_piece][ld_block >= G] */
  const float* V; int64_t ld_v;            /* project: [G][ld_v >= l] */
  float* Y; int64_t ld_y;                  /* project writes, back reads: [n][ld_y >= l] */
  double* Z; int64_t ld_z;                 /* back: [G][ld_z >= l] */
  void* ws; int64_t ws_bytes;              /* back: spv_pca_ws_bytes(G, n_piece, l) bytes or more */
} spv_pca_args;
int spv_pca_stage(const spv_pca_args* a, void* stream);
int spv_pca_project(const spv_pca_args* a, void* stream);
int spv_pca_back(const spv_pca_args* a, void* stream);
/* pure shape functions: the slab of back (it divides 4096); the cell tile of project; the workspace of back in bytes (0 for a
 * non-positive G or n_piece or an l outside the four) */
int32_t spv_pca_slab(void);
int32_t spv_pca_cell_tile(void);
int64_t spv_pca_ws_bytes(int32_t G, int32_t n_piece, int32_t l);

/* Exact t-SNE of a layout of at most SPV_TSNE_DMAX dimensions (spVIPES.latent_tsne / spVIPES.tsne of the user API): three entry points.
 *
 * spv_tsne_repulsion: the all-pairs half of the gradient, nothing of size n_q x n_c stored.  For query row i of Q over the candidates C
 *   Zrow[i] = sum_j (double) w(i, j),   F[t][i] = sum_j (double) fl32(w2(i, j) * fl32(Q[i][t] - C[j][t])),   t < D
 * with d2 the distance of spv_knn above, the same bits, w = fl32(1 / fl32(1 + d2)) (the correctly rounded quotient) and
 * w2 = fl32(w * w).  exclude: int32 [n_q] or NULL, with spv_knn's meaning (candidate exclude[i] is skipped for query i; a value outside
 * [0, n_c) skips nothing).  Layout of F: DIMENSION-MAJOR, fp64 [D][ld_f] with ld_f >= n_q -- F[t * ld_f + i].  Columns >= n_q of F,
 * rows >= n_q and columns >= D of Q / C are never touched.
 * Order of addition: one fp64 running sum per lane and output, ascending j within a chunk of the candidates, ascending chunk across
 * chunks, from +0; no floating-point atomics.  For fixed shapes and n_split two calls agree bit for bit, and a query's sums do not
 * depend on the other queries of the call.  Under DIFFERENT n_split the sums may differ in the last bits of fp64, except where every
 * partial sum is exact.  n_c == 0 gives +0 everywhere.
 * Launches: as spv_knn -- a partial pass of (tiles of spv_knn_tile_q() queries) x (n_split chunks of the candidates) workgroups, and for
 * n_split > 1 a merge pass over the workspace [chunk][1 + D][n_q]; n_split == 1 is ONE launch that writes Zrow / F itself.  n_split = 0
 * stands for spv_tsne_splits(n_q, n_c), a pure function of the shapes.
 * ws: spv_tsne_ws_bytes(n_q, D, n_split) bytes with the RESOLVED n_split (0 for n_split <= 1 or a non-positive shape; 64-bit
 * arithmetic), 8-byte aligned, overwritten by every call.  Nothing is allocated.
 * Rejected ahead of any HIP call with SPV_ERR_ARG: null arguments / Q / C / Zrow / F; ws null when its size is not 0, or not 8-byte
 * aligned; D outside [1, SPV_TSNE_DMAX]; n_split outside [0, SPV_KNN_SPLIT_MAX]; n_q < 1; n_c < 0; ld_q < D; ld_c < D; ld_f < n_q. */
#define SPV_TSNE_DMAX 4
typedef struct spv_tsne_rep_args {
  const float* Q; int64_t ld_q; int32_t n_q;      /* queries    fp32 [n_q][ld_q], ld_q >= D */
  const float* C; int64_t ld_c; int32_t n_c;      /* candidates fp32 [n_c][ld_c], ld_c >= D */
  int32_t D;                                      /* 1 .. SPV_TSNE_DMAX */
  const int32_t* exclude;                         /* [n_q] or NULL */
  int32_t n_split;                                /* 0 = spv_tsne_splits(n_q, n_c); else 1 .. SPV_KNN_SPLIT_MAX chunks of the candidates */
  double* Zrow;                                   /* [n_q] */
  double* F; int64_t ld_f;                        /* [D][ld_f], ld_f >= n_q */
  void* ws;                                       /* spv_tsne_ws_bytes(n_q, D, n_split) bytes */
} spv_tsne_rep_args;
int spv_tsne_repulsion(const spv_tsne_rep_args* a, void* stream);
int32_t spv_tsne_splits(int32_t n_q, int32_t n_c);
int64_t spv_tsne_ws_bytes(int32_t n_q, int32_t D, int32_t n_split);

/* spv_tsne_affinities: the perplexity calibration.  d2 fp32 [n][ld]: per row k squared distances in ascending order as spv_knn returns
 * them, +inf marking an empty slot (idx = -1).  Per row, one lane, fp64: d_j = d2[j] - d2[0]; a binary search for beta from 1, at most 100
 * steps, stopping at |H - log(perplexity)| <= 1e-5, H = log S + beta T / S with S = sum_j e_j, T = sum_j d_j e_j, e_j = exp(-beta d_j) in
 * ascending j; beta doubles (halves) while its upper (lower) bound is infinite, else goes to the midpoint (the search of scikit-learn's
 * _binary_search_perplexity).  P[i][j] = fl32(e_j / S), fp32 [n][ld]; an empty slot gets 0 and does not count; beta fp64 [n].  A row
 * without a finite slot gets zeros and beta = 1.  Columns >= k are never touched.  P may be d2 (in place).
 * Rejected ahead of any HIP call with SPV_ERR_ARG: null d2 / P / beta; n < 1; k outside [1, SPV_KNN_KMAX]; ld < k; perplexity not a
 * finite number >= 1. */
int spv_tsne_affinities(const float* d2, float* P, int64_t ld, int32_t n, int32_t k, double perplexity, double* beta, void* stream);

/* spv_tsne_update: the sparse half of the gradient and the step, two launches.  First ONE workgroup adds Zrow [n] into Z[0] in a fixed
 * order (256 strided lane sums in ascending order, then a pairwise tree).  Then one lane per row i of the symmetric CSR matrix P
 * (indptr int64 [n + 1], cols int32 ascending per row, vals fp32; all on the device; a column outside [0, n) is skipped):
 *   A[t]  = sum_j (double) fl32(fl32(p_ij w_ij) fl32(y_i,t - y_j,t))     in CSR order from +0, w_ij as in spv_tsne_repulsion on y_in
 *   g[t]  = 4 (alpha A[t] - F[t][i] / Z)                                    fp64
 *   gain  = fl32(max(u g < 0 ? gain + 0.2 : gain * 0.8, min_gain)),  u = fl32(momentum u - lr gain g),  y_out = fl32(y_in + u)
 * (scikit-learn's gradient descent step).  y_in / y_out fp32 [n][ld_y], two different arrays: y_in is only read; u and gain fp32
 * [n][ld_y], updated in place.  Optional outputs: kl_row fp64 [n] = sum_j p_ij (log p_ij - log w_ij), so that KL = sum(kl_row) + log Z[0]
 * where the entries of P sum to 1; grad fp64 [D][n] = g.  The order of addition is fixed: two calls on the same inputs agree bit for bit.
 * Rejected ahead of any HIP call with SPV_ERR_ARG: null arguments / y_in / y_out / indptr / cols / vals / Zrow / F / Z / u / gain;
 * y_out == y_in; n < 1; D outside [1, SPV_TSNE_DMAX]; ld_y < D; ld_f < n; alpha, momentum, lr or min_gain negative or not finite. */
typedef struct spv_tsne_upd_args {
  const float* y_in; float* y_out; int64_t ld_y;  /* fp32 [n][ld_y], ld_y >= D */
  int32_t n; int32_t D;                           /* rows; 1 .. SPV_TSNE_DMAX */
  const int64_t* indptr; const int32_t* cols; const float* vals;   /* CSR P */
  const double* Zrow; const double* F; int64_t ld_f;               /* of spv_tsne_repulsion; ld_f >= n */
  double* Z;                                      /* [1], written */
  float* u; float* gain;                          /* [n][ld_y], in place */
  double alpha, momentum, lr, min_gain;           /* exaggeration, momentum, learning rate, floor of the gain */
  double* kl_row;                                 /* [n] or NULL */
  double* grad;                                   /* [D][n] or NULL */
} spv_tsne_upd_args;
int spv_tsne_update(const spv_tsne_upd_args* a, void* stream);

/* The latent gradient of the two rate heads alone: what spv_dec_softmax_bwd computes into dz_part, WITHOUT the in-place correction of
 * tP / tS (a read-only pass: bf16 gradient arrays only).  Lets the caller put the write-back pass, which only the regressor
 * weight-gradient GEMMs wait for, beside the backward pass's critical chain instead of on it. */
int spv_dec_dz(const spv_dec_params* p, const float* Tp, const float* Ts, float* dz_part, void* stream);

/* in place: tP <- tP - softmax_p * Tp[b],  tS <- tS - softmax_s * Ts[b].
 * dz_part (optional, bf16 gradient arrays only): fp32 [gene_splits][Bp][48]; per gene split the gradient reaching the latents
 * through the two rate heads, columns 0..15 = sum_g tP[b][g] * W'_p[g][.], columns 16..47 = sum_g tS[b][g] * W'_s[g][.]
 * (sum the slabs with spv_reduce_slabs): replaces the two [B,G] x [G,K] GEMMs over tP and tS. */
int spv_dec_softmax_bwd(const spv_dec_params* p, const float* Tp, const float* Ts, float* dz_part, void* stream);
/* ONE read-only pass over t_P / t_S (bf16 words, or the hi / lo planes of split-bf16 words when p->grads_f32) for everything the backward pass needs from them (nn/networks.py:314-320 through
 * autograd): the latent gradient of the two rate heads (dz_part, as above) and the two regressor weight gradients
 * d [W'_p | c_p] = t'_P^T [z_p | 1], d [W'_s | c_s] = t'_S^T [z_s | 1] as one partial slab per 128-cell workgroup row:
 * dw_part [Bp / 128][Gp][48], a row = [d W'_p | d c_p | 0.. (16 columns) | d W'_s | d c_s | 0.. (32 columns)] like the regressor operand
 * image (sum the first G rows with spv_reduce_slabs, columns 0..15 and 16..47).  t_P / t_S stay uncorrected -- nothing reads
 * them afterwards: replaces spv_dec_softmax_bwd + spv_dec_heads_wgrad (336 MB less [B, G] traffic per group at B 4096 x G 10 000). */
int spv_dec_heads_bwd(const spv_dec_params* p, const float* Tp, const float* Ts, float* dz_part, float* dw_part, void* stream);

/* One 16-bit operand image kept in step with a parameter by spv_adam_step_images: the `count` fp32 values at flat offset `begin`
 * (a multiple of 4) are a row-major matrix with `cols` columns; element (r, c) is also written to
 * dst[(r + row_off) * ld + c + col_off], rounded to bf16 (fmt SPV_IMAGE_BF16) or as f16(value * scale) (fmt SPV_IMAGE_F16: the fc1
 * weight images, scale = spv_fc1_w_scale()).  A vector that forms one column of an image is cols = 1. */
#define SPV_ADAM_MAX_IMAGES 16
#define SPV_IMAGE_BF16 0
#define SPV_IMAGE_F16 1
typedef struct spv_adam_image {
  int64_t begin, count;
  int32_t cols, row_off, col_off, fmt;
  int64_t ld;
  uint16_t* dst;
  float scale; int32_t _pad;
} spv_adam_image;

/* A range [begin, begin + count) of the flat buffer that spv_adam_step_images leaves alone: p, m, v (and images) there are neither
 * read nor written, because the parameters in it have already taken this step (spv_reduce_slabs_adam).  begin is a multiple of 4
 * (parameters start on 4-element boundaries) and so is count, unless the range ends the buffer. */
#define SPV_ADAM_MAX_SKIP 8
typedef struct spv_adam_range { int64_t begin, count; } spv_adam_range;

/* spv_adam_step that also rewrites the bf16 images of the matrices it updates (the packed operands spv_pack_bf16 would otherwise
 * rebuild at the start of the next step: fc1 weights, [W_m | b_m]).  Image padding (rows / columns outside the matrix) is not
 * touched: the image must have been produced by spv_pack_bf16 once.  n_images may be 0.
 * skip: n_skip <= SPV_ADAM_MAX_SKIP ranges in ascending order, disjoint (n_skip may be 0: every element is updated).  The grid is
 * sized for, and walks, only the elements outside them: a skipped range costs no memory traffic.  An image descriptor that lies in a
 * skipped range is simply never reached. */
int spv_adam_step_images(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                         float weight_decay, float bc1, float bc2, float grad_scale, const spv_adam_image* images, int32_t n_images,
                         const spv_adam_range* skip, int32_t n_skip, int64_t* step_counter, const int64_t* t_dev, double beta1_d,
                         double beta2_d, void* stream);
/* step_counter (nullable): device int64 incremented by one per call (the counter spv_randn / the dropout masks are keyed by).
 * t_dev (nullable): device int64 = optimiser steps ALREADY taken; when given, bc1 / bc2 are ignored and the bias corrections
 * 1 - beta^(t_dev + 1) are formed on the device from beta1_d / beta2_d (double, as torch.optim.Adam forms them on the host): no
 * argument of the launch changes from step to step, so it can be part of the step's captured graph.  The kernel does not write
 * t_dev: advance it with spv_counter_bump after the launch. */

/* Up to SPV_MAXP gathers / copies of 4-byte words in one launch: dst[i] = src[idx ? idx[i] : i], i < count (the minibatch's label
 * gathers, labels[rows] of every group -- the reference's loader does this on the host: data/_multi_datasplitter.py:65-98 -- and the
 * copies of the row indices into the buffers a captured graph reads). */
typedef struct spv_gather_prob { const uint32_t* src; const int32_t* idx; uint32_t* dst; int64_t count; } spv_gather_prob;
int spv_gather_u32(const spv_gather_prob* probs, int32_t nprob, void* stream);

/* n standard-normal draws (the reparameterisation noise of a step: nn/networks.py:128-134, spVIPESmodule.py:346-349 sample with
 * torch's generator) from a counter-based generator: Philox 4x32-10 on (element index / 4, *counter) keyed by `key`, Box-Muller.
 * `counter` (nullable = 0) is read on the device when the kernel runs -- pass the step counter spv_adam_step_images increments and
 * a captured graph draws fresh noise at every replay without any host-side generator state. */
int spv_randn(float* out, int64_t n, const int64_t* counter, uint64_t key, void* stream);
/* *counter += 1 in stream order.  Forward passes that no optimiser step follows (the reference draws fresh torch.randn noise for
 * every batch of get_latent_representation, model/spvipes.py:536-538, nn/networks.py:128-134) advance the counter with this, so
 * that consecutive inference / validation batches do not share one noise matrix. */
int spv_counter_bump(int64_t* counter, void* stream);

/* One Adam step (torch.optim.Adam semantics, L2 weight decay folded into the gradient) over a
 * flat fp32 parameter buffer; grad_scale multiplies g first (1/world for data-parallel means).
 * bc1 = 1 - beta1^t, bc2 = 1 - beta2^t.  Replaces scvi TrainingPlan's optimiser step
 * (constructed at model/base/training_mixin.py:111). */
int spv_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, float bc1, float bc2, float grad_scale,
                  void* stream);

/* ---------------------------------------------------------------------------------------------
 * Small dense primitives for the [B, <=256] layers (encoder tails nn/networks.py:120-129, decoder
 * trunk nn/networks.py:322-323) and their backward.  fp32, batched: one launch serves up to
 * SPV_MAXP independent problems (2 groups x {private, shared} x {mu, logvar} heads).  All arrays row-major.
 * ------------------------------------------------------------------------------------------- */
#define SPV_MAXP 8

typedef struct spv_linear_prob {
  const float* X; int64_t ldx;     /* [B][K]                                     */
  const float* W;                  /* [N][K] (torch Linear weight)               */
  const float* bias;               /* [N] or NULL                                */
  float* Y; int64_t ldy;           /* [B][N] forward output (read again by the backward masks) */
  const float* dY; int64_t lddy;   /* backward: upstream gradient [B][N]         */
  float* dX; int64_t lddx;         /* backward: [B][K]                           */
  float* dW; float* db;            /* backward: [N][K], [N] (db may be NULL)     */
  int32_t N, K;
  const float* keep;               /* forward, drop_p > 0 only: optional [B][N] keep-mask (1 = keep, row pitch N) used INSTEAD of the
                                      counter-based draw -- the dropout mask of nn/networks.py:121 injected by a caller (parity tests) */
  const float* W2; int32_t n_w2;   /* dgrad only, optional: rows n >= n_w2 of the [N][K] weight are W2[n - n_w2] (two layers that read the
                                      same input -- the mu / logvar heads, nn/networks.py:123-124 -- back-propagate into it in ONE launch:
                                      dY = their gradients side by side [B][N], N = the two widths together); W2 == NULL: one matrix */
  /* forward only, optional: Y also as bf16 hi (and lo: split-bf16) words into columns 0..N-1 of a packed operand image [img_rows][ld_img]
   * (the decoder's mixing-logits operand); rows B..img_rows-1 of those columns are zero filled.  img_hi == NULL: no image */
  uint16_t* img_hi; uint16_t* img_lo; int64_t ld_img; int32_t img_rows;
} spv_linear_prob;
typedef struct spv_linear_batch {
  spv_linear_prob p[SPV_MAXP];
  int32_t nprob, B;
  int32_t relu;       /* forward: Y = relu(.); backward: dY masked with (Y > 0)                      */
  float drop_p;       /* inverted dropout after the relu (0 = none); backward rescales where Y > 0   */
  uint64_t seed;      /* counter-based mask: (seed + *seed_ptr, problem, element)                    */
  const uint64_t* seed_ptr; /* optional device-resident addend (lets a captured hipGraph draw fresh masks) */
  int32_t accumulate; /* dgrad: dX += instead of dX =                                                */
} spv_linear_batch;
int spv_linear_fwd(const spv_linear_batch* a, void* stream);    /* Y = dropout(relu(X W^T + b))      */
int spv_linear_dgrad(const spv_linear_batch* a, void* stream);  /* dX (+)= mask(dY) W                */
/* dW = mask(dY)^T X, db = colsum(mask(dY)); wpart: fp32 workspace of >= nprob * 16 * Nmax * (Kmax + 1)
 * elements (the batch is reduced in 16 slices, then summed in slice order)                          */
int spv_linear_wgrad(const spv_linear_batch* a, float* wpart, int64_t wpart_elems, void* stream);

/* A layer's input gradient (batch d: what spv_linear_dgrad computes) and weight gradient (batch w: spv_linear_wgrad) as ONE launch, the
 * input-gradient workgroups first.  The two batches may list different problems (the mu / logvar heads: 8 weight-gradient problems,
 * 4 input-gradient problems with W2 / n_w2); B, relu and drop_p must agree, accumulate belongs to d (w->accumulate must be 0).
 * For B > 256 the launch leaves the 16 slice partials of w in wpart (>= nprob * 16 * Nmax * (Kmax + 1) elements, as for
 * spv_linear_wgrad) and does NOT sum them: describe them with a spv_linear_pending record -- p[i] = w->p[i]'s (dW, db, N, K), nprob,
 * wpart, prob_stride = 16 * Nmax * (Kmax + 1) -- and hand it to the NEXT spv_linear_bwd call on the same stream, whose launch sums them
 * in slice order beside its own work, or to spv_linear_reduce_pending (the last reduction of a chain, or a reduction the next launch
 * waits for).  For B <= 256 the weight gradients are complete after the launch (one slice: no partials, nothing pending).
 * d or w may be NULL (then `pending` rides with one part only; with both NULL the call is spv_linear_reduce_pending).  wpart must not
 * overlap the workspace named in `pending`.
 * THE OUTPUTS OF ONE PART MUST NOT ALIAS THE INPUTS OF THE OTHER (d's dX against w's X / Y / dY, w's dW / db against d's W / W2), nor
 * may the pending dW / db be read by d or w: the parts run concurrently in one grid.  Every result has the bits the separate
 * spv_linear_dgrad / spv_linear_wgrad launches give. */
typedef struct spv_linear_pending_prob { float* dW; float* db; int32_t N, K; } spv_linear_pending_prob;
typedef struct spv_linear_pending {
  spv_linear_pending_prob p[SPV_MAXP];
  int32_t nprob;
  const float* wpart; int64_t prob_stride;   /* problem i's partials: wpart + i * prob_stride, [16][N][K + 1] */
} spv_linear_pending;
int spv_linear_bwd(const spv_linear_batch* d, const spv_linear_batch* w, float* wpart, int64_t wpart_elems,
                   const spv_linear_pending* pending, void* stream);
int spv_linear_reduce_pending(const spv_linear_pending* pending, void* stream);

typedef struct spv_bn_prob {
  const float* X; int64_t ldx;     /* [B][N], N <= 256                                              */
  float* Y; int64_t ldy;
  const float* gamma; const float* beta;
  float* running_mean; float* running_var;   /* updated in training (momentum, unbiased variance)   */
  float* stats;                    /* [N][2] saved (mean, 1/sqrt(var+eps))                          */
  float* part;                     /* workspace [ceil(B/64)][N][2]                                  */
  const float* dY; int64_t lddy;   /* backward                                                     */
  float* dX; int64_t lddx;
  float* dgamma; float* dbeta;
  int32_t N;
  /* optional forward by-product: Y also as a packed bf16 operand image (hi, and lo = bf16(Y - hi) when img_lo != NULL)
   * img[b][c], b < img_rows (rows >= B are written as zeros), c < N, row pitch ld_img                              */
  uint16_t* img_hi; uint16_t* img_lo; int64_t ld_img; int32_t img_rows;
} spv_bn_prob;
typedef struct spv_bn_batch {
  spv_bn_prob p[SPV_MAXP];
  int32_t nprob, B, training, relu;  /* relu: Y = relu(bn(X)) and the backward masks dY with (Y > 0) */
  float eps, momentum;
} spv_bn_batch;
int spv_bn_fwd(const spv_bn_batch* a, void* stream);
int spv_bn_bwd(const spv_bn_batch* a, void* stream);

/* post = BatchNorm output [B][2n] = (loc | logvar): scale = exp(logvar/2), log_z = loc + scale*eps,
 * theta = softmax(log_z), kl_b = KL(N(loc,scale) || N(0,1)) summed over n (nn/networks.py:125-129,
 * module/spVIPESmodule.py:841-854).  Backward: d_post from the (nullable) upstream gradients. */
typedef struct spv_sample_prob {
  const float* post; int32_t n;
  const float* eps;
  float* scale; float* logz; float* theta; float* kl;
  const float* g_loc; const float* g_logvar; const float* g_scale; const float* g_logz; const float* g_kl;
  float* d_post;
  int64_t g_ld;   /* row pitch of g_loc / g_logvar (0 = n): they may be column blocks of a wider matrix */
} spv_sample_prob;
typedef struct spv_sample_batch { spv_sample_prob p[SPV_MAXP]; int32_t nprob, B; } spv_sample_batch;
int spv_enc_sample_fwd(const spv_sample_batch* a, void* stream);
int spv_enc_sample_bwd(const spv_sample_batch* a, void* stream);
/* The encoder heads' BatchNorm + sampling as ONE pair of launches per direction (nn/networks.py:123-129 and its autograd):
 * bn->p[2e], bn->p[2e + 1] = the BatchNorm problems of encoder e's mu / logvar heads (N = n <= 32, their outputs Y the two halves of
 * sb->p[e].post [B][2n], in the backward their dY the two halves of sb->p[e].d_post), sb->p[e] the sampling problem.
 *   forward : bn_stats + one kernel that finalises the statistics, normalises, samples and forms the KL (same bits as
 *             spv_bn_fwd + spv_enc_sample_fwd, two launches fewer)
 *   backward: one kernel for d_post and the BatchNorm partial sums + one that finalises d gamma / d beta and applies
 *             (training-mode statistics only; eval mode: spv_enc_sample_bwd + spv_bn_bwd) */
int spv_enc_heads_fwd(const spv_bn_batch* bn, const spv_sample_batch* sb, void* stream);
int spv_enc_heads_bwd(const spv_bn_batch* bn, const spv_sample_batch* sb, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Label-based Product of Experts on device (module/spVIPESmodule.py:583-718 + _poe2 :282-379).
 * ------------------------------------------------------------------------------------------- */
#define SPV_NB_GSPL_MAX 160 /* genes per likelihood split: their regressor weights sit in LDS */
#define SPV_POE_LMAX 1024   /* label codes are integers in [0, SPV_POE_LMAX) */

/* rank-within-label pairing of two minibatches; labels are float32 codes (as the reference carries
 * them); order*, rank*: int32 scratch [B*]; tables: int32 scratch [2][2][SPV_POE_LMAX];
 * partner*: int32 [B*] (-1 = none); mode*: int32 [B*] (0 partner, 1 ones/zeros padding, 2 label
 * absent from the other group); *err != 0 on a label code outside [0, SPV_POE_LMAX). */
int spv_poe_partner(const float* labels0, const float* labels1, int32_t B0, int32_t B1, int32_t* order0, int32_t* order1,
                    int32_t* rank0, int32_t* rank1, int32_t* tables, int32_t* partner0, int32_t* mode0,
                    int32_t* partner1, int32_t* mode1, int32_t* err, void* stream);

/* the ranking half of spv_poe_partner alone (one launch): rank of every cell within its label, the cells of each label in batch
 * order, tables[2][2][SPV_POE_LMAX] = per group (count, start) per label */
int spv_poe_rank(const float* labels0, const float* labels1, int32_t B0, int32_t B1, int32_t* order0, int32_t* order1,
                 int32_t* rank0, int32_t* rank1, int32_t* tables, int32_t* err, void* stream);

typedef struct spv_poe_args {
  const float* stats[2]; int64_t ld[2];   /* shared encoders' (loc | logvar) rows, [B][ld], logvar at column n */
  const int32_t* partner[2]; const int32_t* mode[2];
  const float* eps[2];                     /* [B][n] */
  float* loc[2]; float* logvar[2]; float* scale[2]; float* logz[2]; float* theta[2]; float* kl[2];
  const float* g_loc[2]; const float* g_logvar[2]; const float* g_scale[2]; const float* g_logz[2]; const float* g_kl[2];
  float* d_stats[2];                       /* backward output, same layout as stats (zeroed by the call itself) */
  int32_t B[2]; int32_t n;
  int32_t clamp_scale;                     /* paired / cluster PoE: the draw and the KL use scale.clamp(min = 1e-6)  */
  int32_t lone_passthrough;                /* cluster PoE: mode 2 keeps the cell's own encoder statistics           */
  const float* expert[2]; int64_t ld_expert[2];  /* cluster PoE: plan-weighted experts [B][ld] (loc | logvar) fused in
                                                    place of the encoder statistics; NULL = label / paired PoE      */
  float* d_expert[2];                      /* backward output for expert (zeroed by the call itself)                */
  /* label PoE: when lab[0] != NULL spv_poe_fuse_fwd derives every cell's partner / mode itself from the ranking left
   * by spv_poe_rank (labels, rank within label, cells of each label in batch order, per-label count / start tables) and STORES them
   * through partner / mode (which are then outputs) for the backward pass -- the separate lookup launch of spv_poe_partner is gone.
   * spv_poe_fuse_bwd reads lab[0] only as a flag: non-NULL = partners are one to one (label pairing: one atomic per cell and column);
   * NULL = partners are arg maxima / component ranks that may coincide (paired, cluster PoE): contributions to one partner are first
   * summed inside a 32-cell workgroup */
  const float* lab[2]; const int32_t* order[2]; const int32_t* rank[2]; const int32_t* tables;
} spv_poe_args;
int spv_poe_fuse_fwd(const spv_poe_args* a, void* stream);
int spv_poe_fuse_bwd(const spv_poe_args* a, void* stream);

/* N-group cluster-matched Product of Experts (BASELINE config 4: 3 groups; the N-expert generalisation of
 * _product_of_experts, module/spVIPESmodule.py:573-581, that SURVEY.md 8d prescribes -- throughput only, the reference stops
 * at two groups: data/prepare_adatas.py:94-95).  For cell i of group g with component c: experts = N(0, 1) prior, the cell's
 * own shared-encoder posterior, and for every other group h with cells of component c in its minibatch the COMPONENT MEAN of
 * h's (loc, logvar).  Fixed-order reductions (no atomics).  Up to SPV_POE_MAXG groups, latent dimension <= 32, component codes
 * integral in [0, ncomp), ncomp <= SPV_POE_COMP_CMAX.                                                                   */
#define SPV_POE_MAXG 4
#define SPV_POE_COMP_SEG 16
#define SPV_POE_COMP_CMAX 64
typedef struct spv_poe_comp_args {
  int32_t ngroups, n, ncomp, pad_;
  int32_t B[SPV_POE_MAXG];
  const float* stats[SPV_POE_MAXG]; int64_t ld[SPV_POE_MAXG];   /* (loc | logvar) rows [B][ld], logvar at column n      */
  const float* comp[SPV_POE_MAXG];                               /* component code of every cell [B] (fp32, integral)     */
  const float* eps[SPV_POE_MAXG];                                /* [B][n] standard-normal draws                         */
  float* part;   /* workspace fp32 [ngroups][SPV_POE_COMP_SEG][ncomp][2n + 1]                                              */
  float* mean;   /* workspace fp32 [ngroups][ncomp][2n + 1]: mean loc | mean logvar | count (kept for the backward pass)   */
  float* loc[SPV_POE_MAXG]; float* logvar[SPV_POE_MAXG]; float* scale[SPV_POE_MAXG]; float* logz[SPV_POE_MAXG];
  float* theta[SPV_POE_MAXG]; float* kl[SPV_POE_MAXG];
  const float* g_loc[SPV_POE_MAXG]; const float* g_logvar[SPV_POE_MAXG]; const float* g_scale[SPV_POE_MAXG];
  const float* g_logz[SPV_POE_MAXG]; const float* g_kl[SPV_POE_MAXG];
  float* dpn[SPV_POE_MAXG];       /* backward workspace [B][2n]                                                           */
  float* d_stats[SPV_POE_MAXG];   /* backward output, layout as stats                                                     */
} spv_poe_comp_args;
int spv_poe_comp_fwd(const spv_poe_comp_args* a, void* stream);
int spv_poe_comp_bwd(const spv_poe_comp_args* a, void* stream);

/* Sparse transport plan: CSR of the plan (rows = dataset cells of group 0, int32 indptr / column
 * indices, fp32 values >= 0) and CSR of its transpose (rows = dataset cells of group 1).  Replaces the dense
 * plan[idx_0][:, idx_1] gather of module/spVIPESmodule.py:474-482.                                                    */
typedef struct spv_plan {
  const int32_t* ptr0; const int32_t* ind0; const float* val0; int32_t n0;   /* plan   : n0 rows */
  const int32_t* ptr1; const int32_t* ind1; const float* val1; int32_t n1;   /* plan^T : n1 rows */
} spv_plan;
/* inv0[c] / inv1[c] = position of dataset cell c in the minibatch (idx0 [B0] / idx1 [B1], unique), -1 if absent */
int spv_plan_invmap(const int32_t* idx0, int32_t B0, const int32_t* idx1, int32_t B1, int32_t* inv0, int32_t n0, int32_t* inv1,
                    int32_t n1, void* stream);
/* paired PoE partners (module/spVIPESmodule.py:520-523): partner0[i] = argmax_j block[i][j], partner1[j] = argmax_i
 * block[i][j] of the minibatch block of the plan; first maximum, 0 for an all-zero row / column                       */
/* Cluster PoE experts (module/spVIPESmodule.py:213-229) from the stored plan entries of the minibatch:
 *   expert[g][i] = sum_j w'_ij * stats[g][j]   (loc | logvar),  j = positions of the other minibatch in i's component,
 *   w' = row-normalised plan weights (row sums clamped at 1e-10, kept in rowsum[g] for the backward).
 * comp[g]: component codes as fp32 [B]; both minibatches have B cells.  The backward ADDS into d_stats[g].            */
typedef struct spv_plan_expert_args {
  spv_plan plan;
  const int32_t* idx[2]; const int32_t* inv[2]; const float* comp[2];
  const float* stats[2]; int64_t ld[2];
  float* expert[2]; int64_t ld_expert[2];
  float* rowsum[2];
  const float* d_expert[2]; float* d_stats[2];
  int32_t B, n;
} spv_plan_expert_args;
int spv_plan_expert_fwd(const spv_plan_expert_args* a, void* stream);
int spv_plan_expert_bwd(const spv_plan_expert_args* a, void* stream);
int spv_plan_argmax(const spv_plan* plan, const int32_t* idx0, const int32_t* idx1, const int32_t* inv0, const int32_t* inv1,
                    int32_t B0, int32_t B1, int32_t* partner0, int32_t* partner1, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Decoder preparation: latent slicing (spVIPESmodule.py:733-754) and BatchNorm folding of the two
 * factor regressors (nn/networks.py:314,318) into the packed operand image of the decoder kernels.
 * ------------------------------------------------------------------------------------------- */
typedef struct spv_zsplit_args {
  const float* priv[2]; const float* poe[2];   /* private log_z [B][n_p], PoE log_z [B][n_s] */
  float* zcat[2];                               /* [B][n_p + n_s] = [z_private | z_shared]    */
  const float* d_zcat[2]; float* d_priv[2]; float* d_poe[2];
  int32_t B, n_p, n_s, ngroups;
  /* optional forward by-products (all rows < Bp, zero beyond B): the decoder's packed bf16 operand images
   *   am  [Bp][ld_am]  columns am_col .. am_col + am_cols - 1  <-  [ zcat | 1 | 0 .. ]   (mixture-logit operand tail)
   *   aps [Bp][48]     <-  [ z_private | 1 | 0 ..(16) | z_shared | 1 | 0 ..(32) ]        (rate-regressor operand)     */
  uint16_t* am_hi[2]; uint16_t* am_lo[2]; int64_t ld_am; int32_t am_col; int32_t am_cols;
  uint16_t* aps_hi[2]; uint16_t* aps_lo[2]; int32_t Bp;
  int32_t kslots;   /* layout of aps: 0 = [Bp][48] as above; 1 = [Bp][96], slots of 32 (private) and 64 (shared) */
} spv_zsplit_args;
int spv_zsplit_fwd(const spv_zsplit_args* a, void* stream);
int spv_zsplit_bwd(const spv_zsplit_args* a, void* stream);

typedef struct spv_fold_prob {
  const float* W; const float* gamma; const float* beta;   /* [G][K], [G], [G]            */
  float* running_mean; float* running_var;                 /* [G]                         */
  const float* zsum; const float* zz;                      /* [K] column sums of z, [K][K] z^T z */
  const float* z; int64_t ldz;                             /* [B][ldz] (backward)         */
  float* stat;                                             /* [G][2] saved (mean, var)    */
  uint16_t* img_hi; uint16_t* img_lo; int64_t ld_img; int32_t col_off; int32_t slot;   /* packed [Gp][ld_img] */
  const float* dWeff; int64_t ld_dw;                       /* backward in: [G][ld_dw], col K = d c */
  float* dW; float* dgamma; float* dbeta;                  /* backward out                */
  float* red_part;                                         /* [ceil(G/256) + 1][K + K*K]  */
  float* dz; int64_t lddz;                                 /* backward out (+=): [B][lddz] */
  int32_t G, Gp, K;
  /* optional: the latent-slicing backward (spVIPESmodule.py:733-754, see spv_zsplit_args) done by the same kernel -- dz then is this
   * problem's column block (first column zcol) of d zcat [B][n_p + n_s], which is only READ, and the finished column c of d zcat goes
   * to d private_log_z / d poe_log_z (out_priv [B][n_p], out_poe [B][n_s]) instead of back into dz: no spv_zsplit_bwd launch.  The two
   * problems of a group (private block, shared block) together cover every column exactly once. */
  int32_t zcol; float* out_priv; float* out_poe; int32_t n_p, n_s;
} spv_fold_prob;
typedef struct spv_fold_batch {
  spv_fold_prob p[SPV_MAXP]; int32_t nprob, B, training; float eps, momentum;
  int32_t kslots;   /* 0: K <= 32; 1 (the wide decoder layout): K <= 64 */
} spv_fold_batch;
int spv_bn_fold_fwd(const spv_fold_batch* a, void* stream);
int spv_bn_fold_bwd(const spv_fold_batch* a, void* stream);   /* fold backward + the z-statistics backward */

/* The decoder's mixing trunk m = relu(BN_256(cat(z) W_a^T + b_a)) (nn/networks.py:322-323; scvi FCLayers: BatchNorm1d eps 1e-3, momentum
 * 0.01) with its training-mode BatchNorm folded the same way: batch mean and variance of a LINEAR map of z follow from zbar and cov(z)
 * (mean_j = w_j . zbar + b_j, var_j = w_j^T C w_j), so the layer is one affine map W'_j = (gamma_j / sqrt(var_j + eps)) w_j,
 * c'_j = beta_j - W'_j . zbar (the Linear's own bias cancels in the batch mean: its gradient is exactly zero, as in the reference) followed
 * by the rectifier: spv_trunk_fold_fwd writes (W', c') for spv_linear_fwd(relu); three launches (statistics, finalise, normalise) and the
 * pre-activation round trip are gone from the forward pass, three (partial sums, finalise, apply) from the backward pass.
 * Backward: from d W' [N][K] and d c' [N] (spv_linear_wgrad of the folded layer, masked by the rectifier) spv_trunk_fold_bwd forms d W_a,
 * d gamma, d beta (d b_a = 0) and (d zbar | d C) [K + K*K], then adds d z[b] += d zbar / B + (d C + d C^T)(z[b] - zbar) / B into dz.
 * Eval mode (training == 0): running statistics instead of batch statistics, no z-statistics term.  N <= 256, K <= 48. */
#define SPV_TRUNK_KMAX 48
typedef struct spv_trunk_prob {
  const float* W; const float* bias; const float* gamma; const float* beta;   /* Linear [N][K], [N]; BatchNorm affine [N], [N]          */
  float* running_mean; float* running_var;                                    /* [N] (updated by the forward call in training mode)    */
  const float* zsum; const float* zz;                                         /* [K] column sums of z, [K][K] z^T z over the batch     */
  float* Wf; float* cf; float* stat;                                          /* forward out: W' [N][K], c' [N], (mean, var) [N][2]    */
  const float* dWf; const float* dcf;                                         /* backward in: d W' [N][K], d c' [N]                    */
  float* dW; float* dbias; float* dgamma; float* dbeta;                       /* backward out: [N][K], [N] (zeros), [N], [N]           */
  float* dred;                                                                /* backward scratch: [ceil(N / 64)][K + K*K] partials of (d zbar | d C) */
  const float* z; int64_t ldz; float* dz; int64_t lddz;                       /* z [B][K] (read), d z [B][K] (accumulated into)        */
  int32_t N, K;
} spv_trunk_prob;
typedef struct spv_trunk_batch { spv_trunk_prob p[2]; int32_t nprob, B, training; float eps, momentum; } spv_trunk_batch;
int spv_trunk_fold_fwd(const spv_trunk_batch* a, void* stream);
int spv_trunk_fold_bwd(const spv_trunk_batch* a, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Deterministic slab reduction (the tail of every split-K GEMM and of the per-wave partials):
 *   dst[r][c] (+)= alpha * escale(c) * sum_s src[s * slab_stride + r * ld_src + col_off + c]
 * up to 8 slabs are added in index order; more than 8 in index order inside four fixed interleaved groups
 * (s = y, y + 4, ...; then ((p0 + p1) + p2) + p3).  rows * cols < 2^31.  alpha: optional device scalar
 * (the upstream gradient of the loss); exp_scale: optional per-column log-scale, multiplies by
 * exp(exp_scale[c]) (d px_r = exp(px_r) * d theta, module/spVIPESmodule.py:758).
 * ------------------------------------------------------------------------------------------- */
#define SPV_MAXR 16
typedef struct spv_reduce_prob {
  const float* src; int64_t slab_stride; int64_t ld_src; int32_t nslabs; int32_t col_off;
  int32_t rows, cols;
  float* dst; int64_t ld_dst; int32_t accumulate; int32_t pad_;
  const float* alpha; const float* exp_scale;
} spv_reduce_prob;
typedef struct spv_reduce_batch { spv_reduce_prob p[SPV_MAXR]; int32_t nprob; } spv_reduce_batch;
int spv_reduce_slabs(const spv_reduce_batch* b, void* stream);

/* Slab sum + Adam in one launch, for a gradient that nothing but the optimiser reads (the mixing head's d W_m / d b_m): per element
 * of problem r (nslabs <= 8, no exp_scale, no accumulate, ld_dst == cols: the gradient slice is the parameter's own contiguous
 * slice of the flat gradient buffer) g = alpha * (slabs in slab order) is stored to r.dst exactly as spv_reduce_slabs stores it, and
 * p, m, v -- the parameter's slices of the flat value / moment buffers, rows * cols elements each -- take the step
 * spv_adam_step_images would take with that g; arguments lr .. beta2_d as there.  img.dst != NULL: the updated value of element
 * (r, c) also goes to img.dst[(r + row_off) * ld + c + col_off] in img.fmt (img.cols == cols, img.count == rows * cols; img.begin
 * is not used).  Word for word the results of spv_reduce_slabs followed by spv_adam_step_images over the same elements.  The launch
 * reads *t_dev and writes neither it nor a step counter: exclude the parameters from the step's spv_adam_step_images call (skip)
 * and advance t_dev once, after that call. */
#define SPV_MAXRA 8
typedef struct spv_reduce_adam_prob { spv_reduce_prob r; float* p; float* m; float* v; spv_adam_image img; } spv_reduce_adam_prob;
typedef struct spv_reduce_adam_batch { spv_reduce_adam_prob p[SPV_MAXRA]; int32_t nprob; } spv_reduce_adam_batch;
int spv_reduce_slabs_adam(const spv_reduce_adam_batch* b, float lr, float beta1, float beta2, float eps, float weight_decay,
                          float bc1, float bc2, float grad_scale, const int64_t* t_dev, double beta1_d, double beta2_d, void* stream);

/* Loss assembly (module/spVIPESmodule.py:870-872): rec_sum = sum_g sum_b w[b] * rec[g][b] and
 *   loss = rec_sum + (kl_weight / B) * sum_b sum_i kl[i][b]   (i < nkl <= 4 KL vectors of length B);
 * also writes gkl[b] = kl_weight / B, the gradient of the loss w.r.t. every kl[i][b].
 * kl_weight is read from device memory (one float) so a captured graph sees later updates. */
int spv_loss_assemble(const float* rec0, const float* rec1, const float* w, const float* const* kl, int32_t nkl, int32_t B,
                      const float* kl_weight, float* loss, float* rec_sum, float* gkl, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPVIPES_HIP_H */
