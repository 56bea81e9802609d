/*
 * coati_search4.h -- four-bit search over an embedding library held in device memory (csrc/search4.hip of libcoati_hip.so): the rows
 * as OCP e2m1 (fp4) nibbles with one E8M0 scale byte per 32 elements (the OCP Microscaling block format), and an approximate
 * streaming stage over them whose candidates coati_search_rescore (coati_search8.h) re-ranks exactly from the bf16 rows.
 *
 * A nineteenth header of the same library and the same conventions as coati_hip.h (which it includes): every function returns 0 or a
 * negative code with a message in coati_last_error(), null pointers and out-of-range arguments are refused before any HIP call, all
 * pointers are DEVICE pointers owned by the caller (PyTorch), `stream` is a hipStream_t passed as void*.  coati_hip.h and
 * COATI_ABI_VERSION are unchanged by it.
 *
 * The reference has no counterpart.
 *
 * Storage: a row of a bf16 library [N, E] (E % 32 == 0) is stored E4 = 128 * ceil(E / 128) elements wide, 128 <= E4 <= 512, the
 * elements at and beyond E taken as zero.  Block b covers elements 32 b .. 32 b + 31.  Its exponent j is the smallest integer with
 * max|x| <= 6 * 2^j, kept within -126 .. 126, 0 for a block of zeros; its scale byte is E8M0 j + 127 in scales [N, E4 / 32] (127 in a
 * pad block; 255 is never written).  An element is x * 2^-j (exact in f32) rounded to the nearest e2m1 value {0, 0.5, 1, 1.5, 2, 3, 4,
 * 6}, ties to the even code; the sign is kept (-0 stays -0); nothing saturates.  The nibble is sign << 3 | code, and byte i of
 * codes [N, E4 / 2] holds element 2 i in its low nibble and element 2 i + 1 in its high one.  Integers from {0, +-1, +-2, +-3, +-4,
 * +-6} times any per-block power of two are stored exactly.  Queries are e4m3 with one power-of-two f32 scale per query
 * (coati_quant_rows_fp8 on the query zero-padded to E4).
 *
 * Limits: 1 <= N < 2^31, Q >= 1, E4 in {128, 256, 384, 512}.
 */
#ifndef COATI_SEARCH4_H
#define COATI_SEARCH4_H

#include "coati_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* codes [n, E4 / 2] and scales [n, E4 / 32] of x [n, E] bf16 by the rule above, E % 32 == 0, 32 <= E <= 512, E4 = 128 * ceil(E / 128):
 * one pass over the rows at their own width, pad nibbles (0) and pad scale bytes (127) included.  Inputs are finite. */
int coati_quant_rows_fp4(const uint16_t* x, int64_t n, int E, uint8_t* codes, uint8_t* scales, void* stream);

/* Stage 1.  Per query i of q8 [Q, E4] e4m3 with qscale [Q]: out_score / out_row [Q, k] = the k best rows of codes [N, E4 / 2] with
 * scales [N, E4 / 32] by (alpha * qscale[i]) * acc + bias[n] (bias [N] f32, required), a zero score canonicalised to +0.  acc is
 * the chain of v_mfma_scale_f32_16x16x128_f8f6f4 results over the E4 / 128 steps in ascending order from a zero accumulator, A =
 * the e4m3 queries with scale byte 127, B = the e2m1 rows with their block scale bytes: the dot product of the query's bytes and
 * the row's dequantised elements, accumulated in f32 (an e4m3 value times an e2m1 value times a power of two is exact in f32).
 * Order, ties, -inf rows, padding, the scratch part_score (f32) / part_row (int32) [Q, S, k] and the independence of S are
 * coati_search_topk's (coati_search.h).  alpha and qscale are expected to be powers of two: the factor is then exact.
 * 1 <= k <= 128, S >= 1, S * k <= 30720. */
int coati_search4_topk(const uint8_t* codes, const uint8_t* scales, int64_t N, int E4, const float* bias, const uint8_t* q8,
                       const float* qscale, int Q, int k, float alpha, int S, float* part_score, int32_t* part_row, float* out_score,
                       int64_t* out_row, void* stream);

/* The S a caller should pass to coati_search4_topk by default (coati_search_slices' arithmetic).  Host arithmetic only, no device call;
 * negative on bad arguments. */
int coati_search4_slices(int64_t N, int Q, int k);

#ifdef __cplusplus
}
#endif

#endif /* COATI_SEARCH4_H */
