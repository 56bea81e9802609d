/*
 * coati_ivf_radius.h -- radius search over an embedding library held in device memory as an inverted file (csrc/ivf_radius.hip of
 * libcoati_hip.so): every row of a query's probed lists within a threshold of the query, in CSR form.  coati_radius.h's answer over
 * coati_ivf.h's storage and work items.
 *
 * A sixteenth header of the same library and the same conventions as coati_hip.h (which it includes): every function returns 0 or a
 * negative code with a message in coati_last_error(), null pointers and out-of-range arguments are refused before any HIP call, all
 * pointers are DEVICE pointers owned by the caller (PyTorch), `stream` is a hipStream_t passed as void*.  coati_hip.h, the other
 * headers and COATI_ABI_VERSION are unchanged by it.
 *
 * The reference has no counterpart.
 *
 * The stored index is coati_ivf.h's, word for word: lib [M, E] bf16 IN LIST ORDER, ids [M] int32 (the original row of every position),
 * bias [M] f32 or null (-inf excludes a row), list_off [L + 1] int32.  PRECONDITION, as there: ids is STRICTLY ASCENDING inside every
 * list.  The pairs are coati_ivf_scan's too: the CALLER inverts the probe table on the device, every (query, list) entry that is not
 * -1 is a PAIR, the P pairs sorted by (list, query) as pair_q [P] / pair_off [L + 1], and item_off [L + 1] is that header's work-item
 * table for seg_rows.  A work item is (list, group of <= 16 of its pairs, segment of seg_rows of its positions); `blocks` workgroups take
 * the items in turn (0 = a default).  segs is the caller's bound on the segments of a list, segs >= ceil(max_l rows_l / seg_rows).
 *
 * The score of (query i, position p) is coati_radius.h's over coati_ivf.h's operands: sc = alpha * dot(q_i, lib_p) + bias[p], the dot
 * accumulated in f32 on the matrix cores in coati_search_topk's k-step order, a zero canonicalised to +0 -- the bits coati_search_topk,
 * coati_ivf_scan and coati_radius_* give the same pair.  The value reported is v = sc - sub[i] (one f32 subtraction; sub [Q] f32, or
 * null for 0), and v = min(v, 0) when clamp0 != 0.  Position p of a list that query i probes is a hit of the pair iff
 *     sc > -inf                                     (a position whose bias is -inf never is, not even at a threshold of -inf),
 *     v >= thr[i]                                   (thr [Q] f32; +inf: the query matches nothing),
 *     ids[p] < row_hi[i]                            (row_hi [Q] int32 over ORIGINAL rows, or null for no bound).
 * Inputs are finite apart from -inf in bias and +-inf in thr; what a NaN does is unspecified.
 *
 * Two passes, as in coati_radius.h: one counts, the caller turns the counts into offsets, one fills.  No atomics, no workspace beyond
 * counts / offsets; where a hit is written depends on the operands and the caller's offsets alone, never on `blocks`, on `seg_rows`,
 * on the stream or on the run.
 *
 * Limits of both passes, those of the two parents: E % 32 == 0, 32 <= E <= 512, 1 <= M < 2^31, 1 <= L <= 4096, 1 <= Q, 1 <= P < 2^31,
 * seg_rows >= 64 and a multiple of 64, segs >= 1, blocks >= 0.
 */
#ifndef COATI_IVF_RADIUS_H
#define COATI_IVF_RADIUS_H

#include "coati_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* counts [P, segs] int32, ZERO-FILLED BY THE CALLER: counts[p, s] = the hits of pair p in segment s of its list.  An entry is written
 * only where a work item covers it and can have a hit: the others -- segments past the end of the pair's list, pairs of a list without
 * rows, segments that begin at or above every row bound of their group -- keep the caller's 0. */
int coati_ivf_radius_count(const uint16_t* lib, const int32_t* ids, const float* bias, const int32_t* list_off, int64_t M, int E, int L,
                           const uint16_t* q, int Q, const int32_t* pair_q, const int32_t* pair_off, const int32_t* item_off, int64_t P,
                           float alpha, const float* sub, int clamp0, const float* thr, const int32_t* row_hi, int seg_rows, int segs,
                           int32_t* counts, int blocks, void* stream);

/* The same operands and the counts coati_ivf_radius_count gave for them; offsets [P, segs] int64: where the hits of (p, s) begin in
 * out_row / out_score, computed by the caller (an exclusive prefix sum of the counts in whatever order of (p, s) it wants the result
 * in; entries whose count is 0 are not read).  The scores are computed again and the hits of (p, s) written at
 * out_row / out_score [offsets[p, s] ...] (int64 ORIGINAL row ids[position], f32 v) in ASCENDING POSITION ORDER, which inside a list is
 * ascending original row.  Nothing is written outside [offsets[p, s], offsets[p, s] + counts[p, s]). */
int coati_ivf_radius_fill(const uint16_t* lib, const int32_t* ids, const float* bias, const int32_t* list_off, int64_t M, int E, int L,
                          const uint16_t* q, int Q, const int32_t* pair_q, const int32_t* pair_off, const int32_t* item_off, int64_t P,
                          float alpha, const float* sub, int clamp0, const float* thr, const int32_t* row_hi, int seg_rows, int segs,
                          const int32_t* counts, const int64_t* offsets, float* out_score, int64_t* out_row, int blocks, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* COATI_IVF_RADIUS_H */
