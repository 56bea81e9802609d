/*
 * coati_guide.h -- the gradient of a property head with respect to its input rows (csrc/guide.hip of libcoati_hip.so): what an optimiser
 * in the embedding space climbs.
 *
 * A sixth header of the same library and the same conventions as coati_hip.h (which coati_screen.h includes): every function returns 0 or
 * a negative code with a message in coati_last_error(), null pointers and out-of-range arguments are refused before any HIP call, all
 * pointers are DEVICE pointers owned by the caller (PyTorch), `stream` is a hipStream_t passed as void*.  coati_hip.h, coati_screen.h, the
 * other headers and COATI_ABI_VERSION are unchanged by it.
 *
 * The head is coati_screen.h's.  It is piecewise linear: the gradient depends on a row only through the D * F ReLU decisions, which the
 * forward records as bits; the backward is the forward's product loop over transposed weights.  One launch, no activation, mask or
 * intermediate gradient in memory, no workspace, no atomics.
 *
 * Arithmetic (coati_amd/models/regression restates it in torch, rounding points included):
 *   forward exactly as coati_head_eval;  m[l] = (rb(h_l) . wr[l]^T + br[l] > 0)   per row and feature, h_l the stream entering block l
 *   out = the same numbers coati_head_eval gives on these rows, bit for bit
 *   d   = cot . wl                                  f32 [F]
 *   d   = d + rb(m[l] (.) d) . wr[l]                l = D - 1 .. 0;  bf16 operands, f32 accumulation, d itself stays f32
 *   g   = rb(d) . w0                                [E]
 * g is the gradient of sum_p cot[p] out[p] with respect to the row as the kernel reads it (the prepared bf16 row); it does not see the
 * rounding of the row to bf16.  What NaN / inf inputs do is unspecified.
 */
#ifndef COATI_GUIDE_H
#define COATI_GUIDE_H

#include "coati_screen.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[n, p] and g[n, e] for n < N, p < P, e < E.  x, w0, b0, wr, br, wl, bl, D, P, F, out, ldo: as in coati_head_eval, the same domain
 * (E % 32 == 0, 32 <= E <= 512;  F in {64, 128, 256};  0 <= D <= 16;  1 <= P <= 8;  1 <= N < 2^31) and the same alignments.
 * w0t [E, F] bf16 is w0 transposed;  wrt [D, F, F] bf16 holds wr[l] transposed (null iff D == 0);  both start at 16-byte boundaries.
 * cot [N, P] f32 is the cotangent, row stride ldc >= P.
 * g [N, E] f32, row stride ldg >= E, ldg % 4 == 0, g 16-byte aligned.
 * Columns E .. ldg-1 of g, columns P .. ldo-1 of out and rows >= N are not written.  g must not overlap x (not checked). */
int coati_head_grad(const uint16_t* x, int64_t ldx, int64_t N, int E,
                    const uint16_t* w0, const float* b0, const uint16_t* wr, const float* br, int D,
                    const float* wl, const float* bl, int P, int F,
                    const uint16_t* w0t, const uint16_t* wrt,
                    const float* cot, int64_t ldc,
                    float* out, int64_t ldo, float* g, int64_t ldg, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* COATI_GUIDE_H */
