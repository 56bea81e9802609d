/*
 * coati_tsne.h -- embedding maps: exact t-SNE of an embedding library in two dimensions (csrc/tsne.hip of libcoati_hip.so).  The
 * conditional probabilities over a kNN graph, the all-pairs repulsive term, and the attraction + gradient + update of one iteration.
 *
 * A twentieth header of the same library and the same conventions as coati_hip.h (which it includes): every function returns 0 or a
 * negative code with a message in coati_last_error(), null pointers and out-of-range arguments are refused before any HIP call, all
 * pointers are DEVICE pointers owned by the caller (PyTorch), `stream` is a hipStream_t passed as void*.  coati_hip.h, the other headers
 * and COATI_ABI_VERSION are unchanged by it.
 *
 * The reference calls sklearn.manifold.TSNE (coati/generative/embed_altair.py); the gradient and the update are sklearn's exact method
 * (_kl_divergence, _gradient_descent) with P restricted to a kNN graph.
 *
 * Everything is f32.  No function uses an atomic, and what each writes is a function of its operands alone: it does not depend on
 * `blocks`, on whether a workspace is given, on the stream or on the run.
 */
#ifndef COATI_TSNE_H
#define COATI_TSNE_H

#include "coati_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per row i of a kNN graph -- d2 [N, k] f32 squared distances (>= 0), nbr [N, k] int32 (-1 = no neighbour: the entry is left out and
 * its p is 0) -- the conditional probabilities p [N, k] f32 of the perplexity `perplexity`, and beta [N] f32 (may be null).
 * With d = d2 - the smallest valid d2 of the row, p(b) = exp(-b d), S = sum p, H(b) = log S + b sum(p d) / S:
 *     b = 1, lo = 0, hi = inf;  `steps` times:  H(b) > log(perplexity) ?  (lo = b;  b = hi is inf ? min(2 b, FLT_MAX) : (b + hi) / 2)
 *                                                                       :  (hi = b;  b = (b + lo) / 2)
 * with no early exit; one more evaluation gives p[i, :] = p(b) / S and beta[i] = b.  A row without a valid entry is zeros, beta 0.
 * The rule ends with finite output whatever the row: equal distances (H is constant: the uniform row), zero distances, fewer valid
 * entries than the perplexity.  One wave per row; the sums of a row are added in a fixed order.
 * 1 <= N < 2^31, 1 <= k <= 128, perplexity > 0 and finite, 0 <= steps <= 10000. */
int coati_tsne_affinities(const float* d2, const int32_t* nbr, int64_t N, int k, float perplexity, int steps, float* p, float* beta,
                          void* stream);

/* For every point i of y [N, 2] f32, over all j != i, with q = 1 / (1 + |y_i - y_j|^2):
 *     rep[i, :] = sum q^2 (y_i - y_j)   ([N, 2] f32),     z[i] = sum q   ([N] f32).
 * The order of the additions: j runs in chunks of J = coati_tsne_chunk() points; a chunk's partial sum starts from zero and takes its
 * j in ascending order; the chunks' partial sums are added in ascending chunk order, starting from zero.  A point that coincides with
 * y_i (j != i) contributes q = 1 and no force.
 * part: null, or f32 scratch of part_floats >= coati_tsne_part_floats(N) elements.  With it, and when the points alone make too few
 * workgroups to fill the device, every (tile of points, chunk) pair is a work item of its own that writes its partial sum to part, and a
 * second launch adds them in chunk order: the same additions in the same order, the same bits.
 * blocks: the workgroups launched, each taking work items in turn; 0 = a default.  The result does not depend on it.
 * 1 <= N < 2^31, blocks >= 0, part_floats >= 0. */
int coati_tsne_repulsion(const float* y, int64_t N, float* rep, float* z, float* part, int64_t part_floats, int blocks, void* stream);

/* J, the points of one chunk of coati_tsne_repulsion.  Host only; it never changes within a build (the summation order hangs on it). */
int coati_tsne_chunk(void);

/* The elements of `part` with which coati_tsne_repulsion may split the chunks over workgroups: 3 N ceil(N / J).  Host arithmetic only, no
 * device call; negative on bad arguments. */
int64_t coati_tsne_part_floats(int64_t N);

/* One iteration's attraction, gradient and update.  The symmetric joint P in CSR: offsets [N + 1] int64 (ascending from 0), cols int32 (in
 * 0 .. N-1, ascending within a row), vals f32.  rep [N, 2], and zsum: a device f32 [1] holding Z = sum z, of coati_tsne_repulsion on y.
 * Per row i, q_e = 1 / (1 + |y_i - y_cols[e]|^2):
 *     att = sum_e vals[e] q_e (y_i - y_cols[e]),     g = 4 (exaggeration att - rep_i / Z)      (rep_i / Z read as 0 where Z is 0)
 * and per coordinate, as sklearn's _gradient_descent:
 *     gain = (update g < 0 ? gain + 0.2 : gain 0.8), floored at min_gain;   update = momentum update - lr gain g;   y_out = y + update
 * update [N, 2] and gains [N, 2] are read and written in place; y_out [N, 2] must not overlap y (other rows read y).
 * kl_rows [N] or null: kl_rows[i] = sum_e vals[e] (log vals[e] - log q_e) over the entries with vals[e] > 0 -- P as given, not
 * exaggerated; KL(P | Q) = sum kl_rows + log Z.  att [N, 2] or null: the row's attraction sum as it entered g.
 * One wave per row: lane l adds the row's entries l, l + 64, ... in that order and the 64 lanes' sums meet in a fixed butterfly, so the
 * bits depend on the row alone, whatever its length (none, or thousands).
 * 1 <= N < 2^31. */
int coati_tsne_step(const float* y, const float* rep, const float* zsum, const int64_t* offsets, const int32_t* cols, const float* vals,
                    int64_t N, float exaggeration, float momentum, float lr, float min_gain, float* update, float* gains, float* y_out,
                    float* kl_rows, float* att, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* COATI_TSNE_H */
