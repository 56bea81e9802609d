/*
 * coati_gp.h -- a Gaussian-process head on inducing points, evaluated on rows of embeddings held in device memory (csrc/gp.hip of
 * libcoati_hip.so): a property head's prediction together with its uncertainty.
 *
 * An eighth header of the same library and the same conventions as coati_hip.h (which it includes): every function returns 0 or a
 * negative code with a message in coati_last_error(), null pointers and out-of-range arguments are refused before any HIP call, all
 * pointers are DEVICE pointers owned by the caller (PyTorch), `stream` is a hipStream_t passed as void*.  coati_hip.h, the other headers
 * and COATI_ABI_VERSION are unchanged by it.
 *
 * The feature extractor is coati_screen.h's FC-ResNet; the GP (an RBF kernel, a constant mean, Mp <= 64 inducing points shared by all P
 * outputs) stands on its last stream.  One kernel carries a tile of rows through every layer and the GP: the library is read once and only
 * [N, P] + [N] floats are written (plus coati_head_eval's [N, P_lin] when wl is given); no feature matrix exists in memory.
 *
 * Arithmetic (coati_amd/models/regression/gp_head.py restates it in torch, rounding points included):
 *   h_D    exactly the stream of coati_head_eval after its D residual blocks;  out = h_D . wl^T + bl as there, bit for bit (wl given)
 *   phi    = rb(h_D)                                the f32 stream rounded to bf16 (nearest even): the GP is DEFINED on phi
 *   d2_j   = max(0, |phi|^2 + zn_j - 2 phi . z_j)   phi . z_j: bf16 operands, f32 accumulation (matrix cores);  |phi|^2 summed in f32 over
 *                                                   the rounded values;  zn_j given by the caller (|z_j|^2 of the bf16 values)
 *   k_j    = s2 * exp(-d2_j * inv2l2)               f32, evaluated as s2 * exp2(d2_j * (-inv2l2 * log2 e)) with the hardware's exp2;
 *                                                   k is NOT rounded
 *   mean_p = c_p + sum_j alpha[p, j] k_j            f32
 *   var    = max(0, s2 - sum_i sum_j k_i q[i, j] k_j)   f32 throughout: w = q k on the f32 matrix cores (v_mfma_f32_32x32x2_f32), then k . w
 * What NaN / inf inputs do is unspecified.
 */
#ifndef COATI_GP_H
#define COATI_GP_H

#include "coati_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mean[n, p] and var[n] for n < N, p < P.  x, ldx, N, E, w0, b0, wr, br, D, F: as in coati_head_eval (coati_screen.h), the same domain
 * (E % 32 == 0, 32 <= E <= 512;  F in {64, 128, 256};  0 <= D <= 16;  1 <= N < 2^31) and the same alignments.
 * wl [P_lin, F] f32, bl [P_lin] f32, out [N, P_lin] f32 with row stride ldo >= P_lin, 1 <= P_lin <= 8: optional.  wl null: bl, P_lin,
 * out and ldo are not looked at.  wl given: bl and out must be given too, and out receives what coati_head_eval writes, bit for bit.
 * z [Mp, F] bf16 row-major inducing points;  zn [Mp] f32;  alpha [P, Mp] f32;  q [Mp, Mp] f32, any matrix (not assumed symmetric);
 * c [P] f32;  z, zn, alpha and q start at 16-byte boundaries.  Mp in {32, 64};  1 <= P <= 8.  Fewer inducing points are padded: a padded
 * point carries zero alpha and a zero row and column of q and then contributes exactly nothing, whatever (finite) z and zn it has.
 * inv2l2 = 1 / (2 l^2) and s2 (the signal variance) are f32 scalars.
 * mean f32, row stride ldm >= P;  var f32 [N].  Columns P .. ldm-1 of mean, columns P_lin .. ldo-1 of out and rows >= N are not written. */
int coati_head_gp(const uint16_t* x, int64_t ldx, int64_t N, int E, const uint16_t* w0, const float* b0,
                  const uint16_t* wr, const float* br, int D, int F,
                  const float* wl, const float* bl, int P_lin, float* out, int64_t ldo,
                  const uint16_t* z, const float* zn, const float* alpha, const float* q, const float* c,
                  float inv2l2, float s2, int P, int Mp,
                  float* mean, int64_t ldm, float* var, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* COATI_GP_H */
