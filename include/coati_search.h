/*
 * coati_search.h -- nearest-neighbour search over an embedding library held in device memory (csrc/search.hip of libcoati_hip.so).
 *
 * A third header of the same library and the same conventions as coati_hip.h (which it includes): every function returns 0 or a
 * negative code with a message in coati_last_error(), null pointers and out-of-range arguments are refused before any HIP call, all
 * pointers are DEVICE pointers owned by the caller (PyTorch), `stream` is a hipStream_t passed as void*.  coati_hip.h, coati_beam.h and
 * COATI_ABI_VERSION are unchanged by it.
 *
 * The reference has no counterpart: its notebooks rank small lists with torch ad hoc.
 *
 * The library is [N, E] bf16 rows, dense and row-major.  The score of (query i, row n) is alpha * dot(q_i, lib_n) + bias[n], the dot
 * accumulated in f32 on the matrix cores; a zero score is canonicalised to +0, so that -0 and +0 tie.  The library is split into S
 * slices of consecutive rows; one kernel streams every slice once per tile of queries and keeps each query's k best in LDS (no score
 * is written to memory), a second one merges the S lists of a query.  The result does not depend on S.
 */
#ifndef COATI_SEARCH_H
#define COATI_SEARCH_H

#include "coati_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per query i of q [Q, E] bf16: out_score / out_row [Q, k] = the k best rows of lib [N, E] bf16 by alpha * dot(q_i, lib_n) + bias[n]
 * (bias [N] f32, or null for none), SCORE DESCENDING, ROW INDEX ASCENDING among equal scores (the order of a stable descending sort).
 * Only rows with a score above -inf are returned: a row whose bias is -inf never is, and when fewer than k rows qualify the tail is
 * (-inf, -1).  Inputs are finite apart from -inf in bias; what a NaN does is unspecified.
 * part_score (f32) / part_row (int32) are [Q, S, k] scratch of the caller.
 * 1 <= k <= 128, E % 32 == 0, 32 <= E <= 512, 1 <= N < 2^31, Q >= 1, S >= 1, S * k <= 30720. */
int coati_search_topk(const uint16_t* lib, int64_t N, int E, const float* bias, const uint16_t* q, int Q, int k, float alpha, int S,
                      float* part_score, int32_t* part_row, float* out_score, int64_t* out_row, void* stream);

/* The S a caller should pass by default: enough slices to fill the device at this Q, no slice shorter than the 64 rows one workgroup
 * takes per iteration, S * k <= 30720.  Host arithmetic only, no device call; negative on bad arguments (the limits above). */
int coati_search_slices(int64_t N, int Q, int k);

#ifdef __cplusplus
}
#endif

#endif /* COATI_SEARCH_H */
