/*
 * coati_ivf.h -- approximate nearest-neighbour search over an embedding library held in device memory as an inverted file (IVF): the
 * rows are stored list by list, a search scores only the rows of every query's probed lists (csrc/ivf.hip of libcoati_hip.so).
 *
 * An eleventh header of the same library and the same conventions as coati_hip.h (which it includes): every function returns 0 or a
 * negative code with a message in coati_last_error(), null pointers and out-of-range arguments are refused before any HIP call, all
 * pointers are DEVICE pointers owned by the caller (PyTorch), `stream` is a hipStream_t passed as void*.  coati_hip.h, coati_search.h,
 * coati_cluster.h, the other headers and COATI_ABI_VERSION are unchanged by it.
 *
 * The reference has no counterpart.
 *
 * The stored index:
 *   lib      [M, E] bf16   the live rows IN LIST ORDER, dense and row-major
 *   ids      [M]    int32  the original library row of every position
 *   bias     [M]    f32    per-position bias, or null for none; -inf excludes a row
 *   list_off [L+1]  int32  list l owns positions list_off[l] .. list_off[l + 1] - 1; list_off[0] = 0, list_off[L] = M, ascending
 * PRECONDITION: ids is STRICTLY ASCENDING inside every list (a stable sort of the rows by list gives that).  The tie rule -- original row
 * ascending among equal scores -- depends on it.
 *
 * The coarse step (which lists a query probes) needs no entry of its own: it is coati_search_topk with the centres as a library of L
 * rows and k = nprobe.  Its result is the probe table [Q, nprobe], -1 where a query probes fewer lists.  A list named twice by one query
 * is the caller's error: what is returned then is unspecified (nothing is written out of bounds).
 *
 * The score of (query i, position p) is alpha * dot(q_i, lib_p) + bias[p], exactly as coati_search_topk computes it: the dot accumulated in
 * f32 on the matrix cores in the same order, a zero canonicalised to +0.  No score matrix is written to memory.  Everything written is a
 * function of the operands alone: it does not depend on `blocks`, on `seg_rows`, on the stream or on the run.
 */
#ifndef COATI_IVF_H
#define COATI_IVF_H

#include "coati_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The scan.  The CALLER inverts the probe table on the device (a stable torch sort): every (query, list) entry that is not -1 is a
 * PAIR, the P pairs sorted by (list, query):
 *   pair_q   [P]   int32  the query of every pair
 *   pair_off [L+1] int32  list l owns pairs pair_off[l] .. pair_off[l + 1] - 1; pair_off[L] <= P
 *   item_off [L+1] int32  the work-item table, item_off[0] = 0 and
 *       item_off[l + 1] = item_off[l] + ceil(pairs_l / 16) * ceil(rows_l / seg_rows)       (0 items if the list has no pairs or no rows)
 * A work item is (list l, group g of <= 16 of its pairs, segment s of seg_rows of its rows); item item_off[l] + s * ceil(pairs_l / 16) + g:
 * consecutive items share the row segment and differ in the pair group.  `blocks` workgroups take the items in turn (0 = a default; the
 * result does not depend on it); a workgroup finds an item's list by bisection of item_off, so no host synchronisation sizes the grid.
 *
 * Written: part_score (f32) / part_row (int32) [P, segs, k]: for pair p and segment s < ceil(rows_l / seg_rows) of its list, the k best
 * positions of the segment by score, SCORE DESCENDING, ORIGINAL ROW ASCENDING among equal scores, the row written being ids[position];
 * padded with (-inf, -1).  Only scores above -inf are candidates.  Slots [p, s, :] with s >= ceil(rows_l / seg_rows), and those of a pair
 * whose list has no rows, are NOT written: coati_ivf_merge does not read them.  segs is the caller's bound on the segments of a list,
 * segs >= ceil(max_l rows_l / seg_rows); a segment s >= segs is not scanned.
 * E % 32 == 0, 32 <= E <= 512, 1 <= M < 2^31, 1 <= L <= 4096, 1 <= Q, 1 <= P < 2^31, 1 <= k <= 128, seg_rows >= 64 and a multiple of 64,
 * segs >= 1, blocks >= 0. */
int coati_ivf_scan(const uint16_t* lib, const int32_t* ids, const float* bias, const int32_t* list_off, int64_t M, int E, int L,
                   const uint16_t* q, int Q, const int32_t* pair_q, const int32_t* pair_off, const int32_t* item_off, int64_t P, int k,
                   float alpha, int seg_rows, int segs, float* part_score, int32_t* part_row, int blocks, void* stream);

/* The merge, one workgroup per query.  probes [Q, nprobe] int32: the probe table (list, or -1); pair_slot [Q, nprobe] int32: the place of
 * that entry's pair in the sorted order (its row of part_*), -1 where probes is -1.  out_score (f32) / out_row (int64) [Q, k] = the k best
 * of the query's partial lists: SCORE DESCENDING, ORIGINAL ROW ASCENDING among equal scores, padded with (-inf, -1).  The selection is on
 * the 64-bit key (order-preserving score key << 32 | ~row).
 * A part slot that no work item wrote does not influence the result: the kernel reads segment s of an entry only for
 * s < ceil(rows_l / seg_rows), computed from list_off -- the caller need not pre-fill part_*.
 * One query's candidates are one row of LDS: nprobe * segs * k <= 16384, refused beyond.  P, seg_rows and segs are the scan's; an
 * entry of pair_slot outside 0 .. P - 1 is taken for -1.
 * 1 <= Q, 1 <= P < 2^31, 1 <= nprobe <= 128, 1 <= k <= 128, 1 <= L <= 4096, seg_rows >= 64 and a multiple of 64, segs >= 1. */
int coati_ivf_merge(const float* part_score, const int32_t* part_row, const int32_t* probes, const int32_t* pair_slot, int64_t P,
                    const int32_t* list_off, int L, int Q, int nprobe, int k, int seg_rows, int segs, float* out_score, int64_t* out_row,
                    void* stream);

/* The seg_rows a caller should pass by default for lists of at most max_list_rows rows: segments short enough that Q * nprobe pairs make
 * enough work items to fill the device at small Q, never below 128 rows, and long enough that nprobe * segs * k <= 16384 holds for
 * segs = ceil(max_list_rows / seg_rows).  A multiple of 64.  Host arithmetic only, no device call; negative on bad arguments (the limits
 * above, 1 <= max_list_rows < 2^31, nprobe * k <= 16384) and where no multiple of 64 below 2^31 holds a segment (max_list_rows above
 * 2^31 - 64 in one segment). */
int64_t coati_ivf_plan(int64_t max_list_rows, int Q, int nprobe, int k);

#ifdef __cplusplus
}
#endif

#endif /* COATI_IVF_H */
