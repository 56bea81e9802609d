/*
 * coati_ln_xhat.h -- the operators behind "a fused LayerNorm saves xhat, not its output" (csrc/gemm_rb16.hip, gemm_ring.hip, gemm.hip of
 * libcoati_hip.so), one by one, as the engine's training step uses them.
 *
 * A seventh header of the same library and the same conventions as coati_hip.h (which it includes): every function returns 0 or a
 * negative code with a message in coati_last_error(), all pointers are DEVICE pointers owned by the caller (PyTorch), `stream` is a
 * hipStream_t passed as void*.  coati_hip.h, the other headers and COATI_ABI_VERSION are unchanged by it.
 *
 * LayerNorm y = xhat gamma + beta with xhat = (x - mean) rstd feeds a Linear (ln_1 -> c_attn, ln_2 -> c_fc of basic_transformer.py:162-174).
 * The forward evaluates the LayerNorm while it loads the product's operand and has to leave a bf16 copy of the rows for the backward.  When
 * that copy is xhat instead of y:
 *   - the LayerNorm's backward, which runs in the write-out of the Linear's input-gradient product, reads 2 bytes of xhat per element where
 *     it read 4 bytes of x (and the row's mean) to rebuild it;
 *   - the Linear's weight gradient streams the same bytes as before and applies gamma / beta to its finished tile:
 *     dW[n, k] = sum_m dY[m, n] y[m, k] = gamma[k] sum_m dY[m, n] xhat[m, k] + beta[k] sum_m dY[m, n].
 */
#ifndef COATI_LN_XHAT_H
#define COATI_LN_XHAT_H

#include "coati_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* g[M, N] (bf16) = NewGELU(LN(x) W^T + bias), codes[M, N] = NewGELU' as 8-bit fixed point (COATI_EPI_GELU_GRAD of coati_gemm_nt), with
 * LN(x) = LayerNorm(x[M, 256] f32, row stride ldx; gamma, beta) evaluated inside the operand load.  mean / rstd [M] receive the row
 * statistics, saved [M, 256] bf16 (row stride 256) the copy for the backward: LN(x) itself (save_xhat = 0) or xhat (save_xhat = 1).
 * g, codes, mean and rstd do not depend on save_xhat, bit for bit.  W [N, 256] bf16 (row stride ldw), N % 16 == 0; the 16-row-slab kernel
 * only: 36 865 .. 65 536 rows, COATI_ESHAPE / COATI_EARG otherwise. */
int coati_gemm_ln_gelu_grad(const float* x, int64_t ldx, const float* gamma, const float* beta, const uint16_t* W, int64_t ldw,
                            const float* bias, int M, int N, uint16_t* saved, float* mean, float* rstd, uint16_t* g, uint8_t* codes,
                            int save_xhat, void* stream);

/* coati_gemm_lnbwd with the LayerNorm's normalised rows read as saved -- xhat [M, 256] bf16, row stride 256 -- instead of being rebuilt
 * from x and mean.  Everything else as coati_gemm_lnbwd (same shapes, same outputs, same optional chained product). */
int coati_gemm_lnbwd_xhat(const uint16_t* dY, int64_t lda, const uint16_t* WT, int64_t ldw, int M, int K, const uint16_t* xhat,
                          const float* rstd, const float* gamma, const float* dres, float* dx, uint16_t* dx16, float* partial,
                          int32_t* n_partial_rows, const uint16_t* chain_W, uint16_t* chain_C, void* stream);

/* coati_wgrad_grouped where problem i's B rows may be the xhat of a LayerNorm whose output is the Linear's real input: with b_gamma[i] /
 * b_beta[i] (f32 [K[i]], both or neither; NULL entries = a plain problem) dW_i[n, k] += b_gamma[i][k] (A_i^T B_i)[n, k] + b_beta[i][k]
 * colsum(A_i)[n]; dbias_i as in coati_wgrad_grouped.  Such a problem needs tile_size 256 and K[i] == 256 (the workgroup that owns a tile
 * then holds its whole column sum): COATI_EARG otherwise.  Workspace: coati_wgrad_grouped_workspace_bytes. */
int coati_wgrad_grouped_affine(int n_problems, const uint16_t* const* A, const int64_t* lda, const uint16_t* const* B, const int64_t* ldb,
                               int M, const int* N, const int* K, float* const* dW, const int64_t* ldw, float* const* dbias,
                               const float* const* b_gamma, const float* const* b_beta, int tile_size, void* workspace,
                               int64_t workspace_bytes, void* stream);

/* What the LayerNorm-fused launches of the engine's last forward left in the saved rows of a transformer pass (0 = encoder pass, 1 =
 * decoder pass): 1 = xhat, 0 = the LayerNorm's output, negative = bad argument.  The engine decides per pass and step (packed-batch row
 * counts on the bf16 path with grouped weight gradients and the LayerNorm backward fused; COATI_NO_LNBWD_FUSE=1 gives 0). */
int coati_engine_ln_saves_xhat(const coati_engine* e, int pass);

#ifdef __cplusplus
}
#endif

#endif /* COATI_LN_XHAT_H */
