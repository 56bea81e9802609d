/*
 * coati_ivfpq.h -- approximate nearest-neighbour search over an inverted file (IVF) whose lists are stored as product-quantisation codes
 * of the RESIDUAL, row minus its list's centre (csrc/ivfpq.hip of libcoati_hip.so): coati_ivf.h's scan over coati_pq.h's storage.
 *
 * An eighteenth header of the same library and the same conventions as coati_hip.h (which it includes): every function returns 0 or a
 * negative code with a message in coati_last_error(), null pointers and out-of-range arguments are refused before any HIP call, all
 * pointers are DEVICE pointers owned by the caller (PyTorch), `stream` is a hipStream_t passed as void*.  coati_hip.h, the other
 * headers and COATI_ABI_VERSION are unchanged by it.
 *
 * The reference has no counterpart.
 *
 * The stored index is coati_ivf.h's with the rows replaced by codes under coati_pq.h's storage rule:
 *   codes    [M, E / 8] uint8   the positions IN LIST ORDER; codes[p][m] names the entry of sub-space m that stands for dimensions
 *                               8 m .. 8 m + 7 of the RESIDUAL of position p (coati_pq_encode of the residuals); 4-byte aligned
 *   ids      [M]    int32       the original library row of every position
 *   bias     [M]    f32         per-position bias, REQUIRED; -inf excludes a row
 *   list_off [L+1]  int32       list l owns positions list_off[l] .. list_off[l + 1] - 1; list_off[0] = 0, list_off[L] = M, ascending
 *   centres  [L, E] bf16        the lists' centres, as the coarse step uses them; 16-byte aligned
 *   codebook [E / 8][256][8] bf16   ONE set of code books for the residuals of all lists; 16-byte aligned
 * The row position p of list l stands for is x_hat[p] = centres[l] + entry(codes[p]); it is never formed.
 * PRECONDITION, as in coati_ivf.h: ids is STRICTLY ASCENDING inside every list.  The tie rule depends on it.
 *
 * No merge, plan or re-scoring entry is declared here: coati_ivf_merge and coati_ivf_plan (coati_ivf.h, the plan called with the number
 * of candidates kept per query in place of k) and coati_search_rescore (coati_search8.h, on the bf16 rows by ORIGINAL row, which is what
 * the merge returns) are used as they are.  The coarse step is coati_search_topk on the centres, as for coati_ivf_scan.
 */
#ifndef COATI_IVFPQ_H
#define COATI_IVFPQ_H

#include "coati_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The scan over lists of residual codes.  q [Q, E] bf16.  The score of (the pair of query i with list l, position p of that list) is
 * alpha * acc + bias[p], a zero canonicalised to +0, where acc is ONE f32 v_mfma_f32_16x16x32_bf16 chain from zero: first the E / 32
 * k-steps of centres[l] against q_i in ascending order, then the E / 32 k-steps of the code-book entries of codes[p] against q_i again.
 * That is, bit for bit, what coati_ivf_scan returns at width 2 E for the library row [centres[l] | entry(codes[p])] and the query
 * [q_i | q_i] under the same tables.  The centre's half of the chain is computed once per work item, not per position.
 *
 * EVERYTHING ELSE IS coati_ivf_scan's contract (coati_ivf.h), word for word: the pair table pair_q [P] / pair_off [L+1] sorted by
 * (list, query), the work-item table item_off [L+1] and the numbering of the items (segment-major, groups of <= 16 pairs), `blocks`;
 * what is written to part_score (f32) / part_row (int32) [P, segs, k] and which slots are NOT written; score descending, original row
 * ascending among equal scores (through the precondition on ids), the row written being ids[position]; padding with (-inf, -1); only
 * scores above -inf are candidates; and the independence of everything written from `blocks`, `seg_rows`, the stream and the run.
 * No atomics to memory, no score matrix.
 * A workgroup holds the whole code book (512 E bytes) in LDS, copied once before its first work item, next to the lists of an item's 16
 * pairs; blocks = 0 is therefore at most one workgroup per compute unit.
 * E % 32 == 0, 32 <= E <= 256, 1 <= k <= coati_ivfpq_k_max(E), and coati_ivf_scan's limits otherwise: 1 <= M < 2^31, 1 <= L <= 4096,
 * 1 <= Q, 1 <= P < 2^31, seg_rows >= 64 and a multiple of 64, segs >= 1, blocks >= 0. */
int coati_ivfpq_scan(const uint8_t* codes, const int32_t* ids, const float* bias, const int32_t* list_off, int64_t M, int E, int L,
                     const uint16_t* centres, const uint16_t* codebook, const uint16_t* q, int Q, const int32_t* pair_q,
                     const int32_t* pair_off, const int32_t* item_off, int64_t P, int k, float alpha, int seg_rows, int segs,
                     float* part_score, int32_t* part_row, int blocks, void* stream);

/* The largest k coati_ivfpq_scan takes at this E: the code book (512 E bytes), the lists of a work item's 16 pairs (16 * (k + 128) * 8
 * bytes) and 16 * 8 + 8 bytes of counts, thresholds and flags fit 160 KiB at k = 128 for every E <= 224; at E = 256 (128 KiB of code
 * book) k = 64 fits, with 24 KiB of lists.  Host arithmetic only, no device call; negative on a bad E. */
int coati_ivfpq_k_max(int E);

#ifdef __cplusplus
}
#endif

#endif /* COATI_IVFPQ_H */
