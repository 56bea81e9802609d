/*
 * coati_cluster.h -- clustering of an embedding library held in device memory (csrc/cluster.hip of libcoati_hip.so): every row's nearest
 * centre, and the per-cluster sums of the rows -- the two passes of a Lloyd round.
 *
 * A tenth header of the same library and the same conventions as coati_hip.h (which it includes): every function returns 0 or a negative
 * code with a message in coati_last_error(), null pointers and out-of-range arguments are refused before any HIP call, all pointers are
 * DEVICE pointers owned by the caller (PyTorch), `stream` is a hipStream_t passed as void*.  coati_hip.h, coati_search.h, the other headers
 * and COATI_ABI_VERSION are unchanged by it.
 *
 * The reference has no counterpart.
 *
 * The library is [N, E] bf16 rows, dense and row-major, as in coati_search.h.  Neither function writes a score matrix, neither uses an
 * atomic, and what each writes is a function of its operands alone: it does not depend on `blocks`, the stream or the run.
 */
#ifndef COATI_CLUSTER_H
#define COATI_CLUSTER_H

#include "coati_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per row n of lib [N, E] bf16: assign[n] (int32) = the centre k of c [K, E] bf16 that maximises dot(lib_n, c_k) + cbias[k] (cbias [K]
 * f32, or null for none), the dot accumulated in f32 on the matrix cores; among equal scores the SMALLEST k.  best[n] (f32) = that score,
 * a zero canonicalised to +0.  row_bias [N] f32 or null: a row whose entry is -inf is excluded -- assign[n] = -1, best[n] = -inf -- and any
 * other value is ignored.  Inputs are finite apart from that; what a NaN or an infinite cbias does is unspecified.
 * The library is read once; the centres pass through LDS in tiles of 32 in ascending order.
 * blocks: the workgroups launched, each taking whole tiles of rows in turn; 0 = one per tile of rows.  The result does not depend on it.
 * E % 32 == 0, 32 <= E <= 512, 1 <= N < 2^31, 1 <= K <= 4096, blocks >= 0. */
int coati_cluster_assign(const uint16_t* lib, int64_t N, int E, const float* row_bias, const uint16_t* c, int K, const float* cbias,
                         int32_t* assign, float* best, int blocks, void* stream);

/* sums [K, E] f32: sums[k] = the sum of the library rows of cluster k, zeros for an empty cluster.
 * order [M] int32: the rows that take part, sorted by (cluster, row) -- the indices of a stable sort of assign with the excluded rows
 * left out; an entry outside 0 .. N-1 is read as row 0.  offsets [K + 1] int32: cluster k owns order[offsets[k] .. offsets[k + 1] - 1],
 * offsets[0] = 0, offsets[K] = M, ascending.
 * Every cluster's list is cut into chunks of CH = coati_cluster_chunk() rows; a chunk is one work item, the items numbered cluster by
 * cluster, chunk by chunk.  The item table is item_off [K + 1] int32, built by the CALLER (on the device, three torch calls):
 *     item_off[0] = 0,   item_off[k + 1] = item_off[k] + ceil((offsets[k + 1] - offsets[k]) / CH)
 * so item i with item_off[k] <= i < item_off[k + 1] is chunk j = i - item_off[k] of cluster k: rows order[offsets[k] + j CH ..] up to the
 * end of the chunk or of the cluster.  The first launch writes part[i, :] (f32 [items_max, E], scratch of the caller, items_max >=
 * coati_cluster_items_max(M, K) >= item_off[K]) = the sum of item i's rows in a fixed order; the second adds every cluster's partial rows
 * in chunk order into sums.  The order of every addition is a function of offsets and CH alone.
 * blocks: the workgroups of the first launch, each taking items in turn; 0 = a default.  The result does not depend on it.
 * E % 32 == 0, 32 <= E <= 512, 1 <= N < 2^31, 1 <= K <= 4096, 1 <= M <= N, blocks >= 0. */
int coati_cluster_sums(const uint16_t* lib, int64_t N, int E, const int32_t* order, int64_t M, const int32_t* offsets,
                       const int32_t* item_off, int K, float* part, int64_t items_max, float* sums, int blocks, void* stream);

/* CH, the rows of one work item of coati_cluster_sums.  Host only; it never changes within a build (the summation order hangs on it). */
int coati_cluster_chunk(void);

/* The most work items that M rows in K clusters can make, floor(M / CH) + K: the rows that part needs.  Host arithmetic only, no device
 * call; negative on bad arguments (the limits above, M >= 0). */
int64_t coati_cluster_items_max(int64_t M, int K);

#ifdef __cplusplus
}
#endif

#endif /* COATI_CLUSTER_H */
