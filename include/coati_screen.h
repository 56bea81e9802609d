/*
 * coati_screen.h -- property heads evaluated on rows of embeddings held in device memory (csrc/screen.hip of libcoati_hip.so).
 *
 * A fifth header of the same library and the same conventions as coati_hip.h (which it includes): every function returns 0 or a
 * negative code with a message in coati_last_error(), null pointers and out-of-range arguments are refused before any HIP call, all
 * pointers are DEVICE pointers owned by the caller (PyTorch), `stream` is a hipStream_t passed as void*.  coati_hip.h, the other headers
 * and COATI_ABI_VERSION are unchanged by it.
 *
 * The head is the deterministic part of the reference's regressors (coati.models.regression): the FC-ResNet feature extractor with a
 * linear last layer.  One kernel carries a tile of rows through every layer: the library is read once and only [N, P] floats are written.
 *
 * Arithmetic (coati_amd/models/regression restates it in torch, rounding points included):
 *   h   = x . w0^T + b0                         bf16 operands, f32 accumulation, f32 result
 *   h   = h + relu(rb(h) . wr[l]^T + br[l])     l = 0 .. D - 1;  rb rounds the f32 stream to bf16 (nearest even) for the product's
 *                                               operand only, the residual stream h itself stays f32
 *   out = h . wl^T + bl                         f32, on the unrounded h
 * What NaN / inf inputs do is unspecified.
 */
#ifndef COATI_SCREEN_H
#define COATI_SCREEN_H

#include "coati_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[n, p] for n < N, p < P.  x [N, E] bf16 rows, stride ldx elements (ldx >= E, ldx % 8 == 0, x 16-byte aligned).
 * w0 [F, E] bf16 row-major (torch Linear layout), b0 [F] f32;  wr [D, F, F] bf16, br [D, F] f32 (null iff D == 0);
 * wl [P, F] f32, bl [P] f32;  out f32, row stride ldo >= P; columns P .. ldo-1 and rows >= N are not written.
 * E % 32 == 0, 32 <= E <= 512;  F in {64, 128, 256};  0 <= D <= 16;  1 <= P <= 8;  1 <= N < 2^31.
 * w0, b0, wr, br and wl start at 16-byte boundaries. */
int coati_head_eval(const uint16_t* x, int64_t ldx, int64_t N, int E, const uint16_t* w0, const float* b0,
                    const uint16_t* wr, const float* br, int D, const float* wl, const float* bl, int P, int F,
                    float* out, int64_t ldo, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* COATI_SCREEN_H */
