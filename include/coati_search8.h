/*
 * coati_search8.h -- quantised search over an embedding library held in device memory (csrc/search8.hip of libcoati_hip.so): the rows
 * as OCP e4m3 bytes plus one scale per row, an approximate streaming stage over them, and an exact re-ranking of its candidates from
 * the bf16 rows.
 *
 * A fourteenth header of the same library and the same conventions as coati_hip.h (which it includes): every function returns 0 or a
 * negative code with a message in coati_last_error(), null pointers and out-of-range arguments are refused before any HIP call, all
 * pointers are DEVICE pointers owned by the caller (PyTorch), `stream` is a hipStream_t passed as void*.  coati_hip.h and
 * COATI_ABI_VERSION are unchanged by it.
 *
 * The reference has no counterpart.
 *
 * Storage: row n of a bf16 library [N, E] is x_n / s_n rounded to e4m3 (e4m3fn: no infinities, largest value 448; round to nearest
 * even) with s_n = 2^j, j the smallest integer such that max|x_n| <= 448 * 2^j (j kept within -126 .. 127; s_n = 1 for a row of
 * zeros).  Nothing saturates, -0 stays -0, and a row that e4m3 holds exactly after the scaling -- integers of magnitude <= 15, for one
 * -- is stored exactly.  Scales are f32, one per row.  Queries are quantised the same way, one scale per query.
 *
 * Limits of every entry: E % 32 == 0, 32 <= E <= 512, 1 <= N < 2^31, Q >= 1.
 */
#ifndef COATI_SEARCH8_H
#define COATI_SEARCH8_H

#include "coati_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out [n, E] e4m3 bytes and scale [n] f32 of x [n, E] bf16, by the rule above: bit for bit torch's
 * (x.float() / scale[:, None]).to(torch.float8_e4m3fn).  One pass, one wave per row.  Inputs are finite. */
int coati_quant_rows_fp8(const uint16_t* x, int64_t n, int E, uint8_t* out, float* scale, void* stream);

/* Stage 1.  Per query i of q8 [Q, E] e4m3 with qscale [Q]: out_score / out_row [Q, k] = the k best rows of lib8 [N, E] e4m3 with
 * scale [N] by (alpha * qscale[i] * scale[n]) * dot(q8_i, lib8_n) + bias[n] (bias [N] f32, required), the dot accumulated in f32
 * on the matrix cores (v_mfma_f32_16x16x32_fp8_fp8; a product of two e4m3 values is exact in f32), a zero score canonicalised to +0.
 * Order, ties, -inf rows, padding, the scratch part_score (f32) / part_row (int32) [Q, S, k] and the independence of S are
 * coati_search_topk's (coati_search.h).  alpha and the scales are expected to be powers of two: the factor is then exact.
 * 1 <= k <= 128, S >= 1, S * k <= 30720. */
int coati_search8_topk(const uint8_t* lib8, const float* scale, int64_t N, int E, const float* bias, const uint8_t* q8, const float* qscale,
                       int Q, int k, float alpha, int S, float* part_score, int32_t* part_row, float* out_score, int64_t* out_row,
                       void* stream);

/* Stage 2.  cand [Q, R] int64: per query R candidate rows of lib [N, E] bf16, distinct, in any order; an entry outside 0 .. N - 1
 * (-1 by convention) is no candidate.  Each is scored against q [Q, E] bf16 with coati_search_topk's arithmetic -- alpha * dot + bias[row],
 * the dot on v_mfma_f32_16x16x32_bf16 over the k-steps in ascending order from a zero accumulator, a zero canonicalised to +0: the BITS
 * coati_search_topk gives the same (query, row) -- and out_score / out_row [Q, k] are the best k by (score descending, row ascending),
 * padded with (-inf, -1).  A candidate whose bias is -inf is not a result.  One launch, one workgroup per query.
 * 1 <= R <= 128, 1 <= k <= 128. */
int coati_search_rescore(const uint16_t* lib, int64_t N, int E, const float* bias, const uint16_t* q, int Q, const int64_t* cand, int R, int k,
                         float alpha, float* out_score, int64_t* out_row, void* stream);

/* The S a caller should pass to coati_search8_topk by default (coati_search_slices' arithmetic).  Host arithmetic only, no device call;
 * negative on bad arguments. */
int coati_search8_slices(int64_t N, int Q, int k);

#ifdef __cplusplus
}
#endif

#endif /* COATI_SEARCH8_H */
