/*
 * coati_ivf8.h -- approximate nearest-neighbour search over an inverted file (IVF) whose lists are stored as OCP e4m3 bytes plus one
 * scale per row (csrc/ivf8.hip of libcoati_hip.so): coati_ivf.h's scan over coati_search8.h's storage.
 *
 * A fifteenth header of the same library and the same conventions as coati_hip.h (which it includes): every function returns 0 or a
 * negative code with a message in coati_last_error(), null pointers and out-of-range arguments are refused before any HIP call, all
 * pointers are DEVICE pointers owned by the caller (PyTorch), `stream` is a hipStream_t passed as void*.  coati_hip.h, the other
 * headers and COATI_ABI_VERSION are unchanged by it.
 *
 * The reference has no counterpart.
 *
 * The stored index is coati_ivf.h's with the rows quantised by coati_search8.h's rule (coati_quant_rows_fp8):
 *   lib8     [M, E] uint8  the live rows IN LIST ORDER as e4m3 bytes, dense and row-major
 *   scale    [M]    f32    the positions' scales, powers of two
 *   ids      [M]    int32  the original library row of every position
 *   bias     [M]    f32    per-position bias, REQUIRED; -inf excludes a row
 *   list_off [L+1]  int32  list l owns positions list_off[l] .. list_off[l + 1] - 1; list_off[0] = 0, list_off[L] = M, ascending
 * PRECONDITION, as in coati_ivf.h: ids is STRICTLY ASCENDING inside every list.  The tie rule depends on it.
 *
 * No merge, plan or re-scoring entry is declared here: coati_ivf_merge and coati_ivf_plan (coati_ivf.h, the plan called with the number
 * of candidates kept per query in place of k) and coati_search_rescore (coati_search8.h, on the bf16 rows by ORIGINAL row, which is what
 * the merge returns) are used as they are.  The coarse step is coati_search_topk on the centres, as for coati_ivf_scan.
 */
#ifndef COATI_IVF8_H
#define COATI_IVF8_H

#include "coati_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The scan over fp8 lists.  q8 [Q, E] e4m3 and qscale [Q] f32 are the quantised queries and their scales (coati_quant_rows_fp8).
 * The score of (query i, position p) is coati_search8_topk's: (alpha * qscale[i] * scale[p]) * dot(q8_i, lib8_p) + bias[p], the dot
 * accumulated in f32 on the matrix cores (v_mfma_f32_16x16x32_fp8_fp8) in the order coati_search8_topk uses, a zero canonicalised to
 * +0: a (query, row) pair has the same bits in both.  alpha and the scales are expected to be powers of two.
 *
 * EVERYTHING ELSE IS coati_ivf_scan's contract (coati_ivf.h), word for word: the pair table pair_q [P] / pair_off [L+1] sorted by
 * (list, query), the work-item table item_off [L+1] and the numbering of the items (segment-major, groups of <= 16 pairs), `blocks`;
 * what is written to part_score (f32) / part_row (int32) [P, segs, k] and which slots are NOT written; score descending, original row
 * ascending among equal scores (through the precondition on ids), the row written being ids[position]; padding with (-inf, -1); only
 * scores above -inf are candidates; and the independence of everything written from `blocks`, `seg_rows`, the stream and the run.
 * The limits are coati_ivf_scan's too: E % 32 == 0, 32 <= E <= 512, 1 <= M < 2^31, 1 <= L <= 4096, 1 <= Q, 1 <= P < 2^31,
 * 1 <= k <= 128, seg_rows >= 64 and a multiple of 64, segs >= 1, blocks >= 0. */
int coati_ivf8_scan(const uint8_t* lib8, const float* scale, const int32_t* ids, const float* bias, const int32_t* list_off, int64_t M, int E,
                    int L, const uint8_t* q8, const float* qscale, int Q, const int32_t* pair_q, const int32_t* pair_off,
                    const int32_t* item_off, int64_t P, int k, float alpha, int seg_rows, int segs, float* part_score, int32_t* part_row,
                    int blocks, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* COATI_IVF8_H */
