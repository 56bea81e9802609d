/*
 * coati_radius.h -- radius search over an embedding library held in device memory (csrc/radius.hip of libcoati_hip.so): every row
 * within a threshold of each query, in CSR form.
 *
 * A twelfth header of the same library and the same conventions as coati_hip.h (which it includes): every function returns 0 or a
 * negative code with a message in coati_last_error(), null pointers and out-of-range arguments are refused before any HIP call, all
 * pointers are DEVICE pointers owned by the caller (PyTorch), `stream` is a hipStream_t passed as void*.  coati_hip.h and
 * COATI_ABI_VERSION are unchanged by it.
 *
 * The reference has no counterpart: its notebooks rank small lists with torch ad hoc.
 *
 * The library is [N, E] bf16 rows, dense and row-major, as in coati_search.h, and the score of (query i, row n) is that header's:
 * sc = alpha * dot(q_i, lib_n) + bias[n], the dot accumulated in f32 on the matrix cores in the same k-step order, a zero canonicalised
 * to +0 -- the bits coati_search_topk gives the same pair.  The value reported is v = sc - sub[i] (one f32 subtraction; sub [Q] f32, or
 * null for 0), and v = min(v, 0) when clamp0 != 0.  Row n is a hit of query i iff
 *     sc > -inf                                     (a row whose bias is -inf never is, not even at a threshold of -inf),
 *     v >= thr[i]                                   (thr [Q] f32; +inf: the query matches nothing),
 *     n < row_hi[i]                                 (row_hi [Q] int32, or null for no bound).
 * Inputs are finite apart from -inf in bias and +-inf in thr; what a NaN does is unspecified.
 *
 * The answer's size is known only after a scan, so there are two passes over the library's S slices (consecutive row ranges of whole
 * 64-row iterations, as in the search): one counts, the caller turns the counts into offsets, one fills.  No atomics, no workspace
 * beyond counts / offsets; the position of every hit depends on the data alone, never on S or the launch.
 *
 * Limits of both passes: E % 32 == 0, 32 <= E <= 512, 1 <= N < 2^31, Q >= 1, 1 <= S <= 65535.
 */
#ifndef COATI_RADIUS_H
#define COATI_RADIUS_H

#include "coati_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* counts [Q, S] int32 = the hits of query i of q [Q, E] bf16 in slice s of lib [N, E] bf16.  Every entry is written. */
int coati_radius_count(const uint16_t* lib, int64_t N, int E, const float* bias, const uint16_t* q, int Q, float alpha, const float* sub,
                       int clamp0, const float* thr, const int32_t* row_hi, int S, int32_t* counts, void* stream);

/* The same operands and the counts coati_radius_count gave for them; offsets [Q * S] int64 = the exclusive prefix sum of counts
 * flattened in (query, slice) order, computed by the caller.  The scores are computed again and the hits of (i, s) written at
 * out_row / out_score [offsets[i * S + s] ...] (int64 row, f32 v) in ASCENDING ROW ORDER: a query's results are contiguous and
 * row-ascending whatever S is.  Nothing is written outside [offsets[i * S + s], offsets[i * S + s] + counts[i * S + s]). */
int coati_radius_fill(const uint16_t* lib, int64_t N, int E, const float* bias, const uint16_t* q, int Q, float alpha, const float* sub,
                      int clamp0, const float* thr, const int32_t* row_hi, int S, const int32_t* counts, const int64_t* offsets,
                      float* out_score, int64_t* out_row, void* stream);

/* The S a caller should pass by default: enough slices to fill the device at this Q, no slice shorter than the 64 rows one workgroup
 * takes per iteration, at most 65535 (the grid's y limit).  Host arithmetic only, no device call; negative on bad arguments. */
int coati_radius_slices(int64_t N, int Q);

#ifdef __cplusplus
}
#endif

#endif /* COATI_RADIUS_H */
