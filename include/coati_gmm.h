/*
 * coati_gmm.h -- a mixture of K diagonal Gaussians over an embedding library held in device memory (csrc/gmm.hip of libcoati_hip.so):
 * every row's log-density and most responsible component (the E-step), and the responsibility-weighted zeroth, first and second moments of
 * the rows (the M-step) -- the two passes of an EM iteration.
 *
 * A twenty-first header of the same library and the same conventions as coati_hip.h (which it includes): every function returns 0 or a
 * negative code with a message in coati_last_error(), null pointers and out-of-range arguments are refused before any HIP call, all
 * pointers are DEVICE pointers owned by the caller (PyTorch), `stream` is a hipStream_t passed as void*.  coati_hip.h, coati_cluster.h, the
 * other headers and COATI_ABI_VERSION are unchanged by it.
 *
 * The reference has no counterpart (its density is one full-covariance Gaussian fitted in torch).
 *
 * Operands of both functions: lib [N, E] bf16 rows, dense and row-major, as in coati_cluster.h; row_bias [N] f32 or null -- a row whose
 * entry is -inf is excluded, any other value is ignored; par [K, 2E] f32 with par[k, :E] = mu_k / var_k and par[k, E:] = -0.5 / var_k;
 * cst [K] f32.  The logit of row n under component k is
 *     logit[n, k] = sum_d (x_nd par[k, d] + x_nd^2 par[k, E + d]) + cst[k]
 * with the bf16 rows widened exactly, x^2 taken in f32 (exact: 16 significant bits) and both sums accumulated in f32 on the f32 matrix
 * cores (v_mfma_f32_16x16x4_f32), the linear and the quadratic half in an accumulator each, added once, then cst.  With
 * cst[k] = log w_k - sum_d (mu^2 / var + log(2 pi var)) / 2 that is log(w_k N(x_n | mu_k, diag var_k)); the kernels know nothing of
 * weights, variances or padded columns (a padded column has par = 0).  Inputs are finite; what a NaN does is unspecified.
 * Neither function writes an [N, K] matrix, neither uses an atomic, and what each writes is a function of its operands alone: it does
 * not depend on `blocks`, the stream or the run.
 * E % 32 == 0, 32 <= E <= 512, 1 <= N < 2^31, 1 <= K <= 256, blocks >= 0.
 */
#ifndef COATI_GMM_H
#define COATI_GMM_H

#include "coati_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lse[n] (f32) = log sum_k exp(logit[n, k]), computed online as a running maximum and a scaled sum: finite however negative every logit
 * is (a logit below -FLT_MAX counts as -FLT_MAX).  assign[n] (int32; assign may be null) = the k of the largest logit, the SMALLEST k
 * among equal ones.  An excluded row gets lse = -inf, assign = -1.
 * The library is read once; the parameter rows pass through LDS in tiles of 16 components in ascending order, a lane meets its components
 * in ascending order and the 16 lanes of a row combine in a fixed order.
 * blocks: the workgroups launched, each taking whole tiles of rows in turn; 0 = a default.  The result does not depend on it. */
int coati_gmm_estep(const uint16_t* lib, int64_t N, int E, const float* row_bias, const float* par, int K, const float* cst, float* lse,
                    int32_t* assign, int blocks, void* stream);

/* With r[n, k] = exp(logit[n, k] - lse[n]) (0 for an excluded row; the logit recomputed by the E-step's own device function, so bit for
 * bit the one lse was made from), writes w [K] = sum_n r, s1 [K, E] = sum_n r x_nd and s2 [K, E] = sum_n r x_nd^2, all f32, the two
 * products on the f32 matrix cores with r kept in f32.
 * The rows are cut into chunks of CH = coati_gmm_chunk() rows and the ceil(N / CH) chunks into R = coati_gmm_ranges(N) contiguous ranges,
 * range i owning chunks floor(i chunks / R) .. floor((i + 1) chunks / R) - 1.  A work item is (range, tile of 16 components): it adds
 * its rows in ascending order in registers and writes one block of part (f32 scratch of the caller, part_floats >=
 * coati_gmm_part_floats(N, E, K)); a second launch adds the ranges in ascending order.  The order of every addition is a function of
 * (N, E, K) and the build's constants alone.
 * blocks: the workgroups of the first launch, each taking items in turn; 0 = one per item.  The result does not depend on it. */
int coati_gmm_mstep(const uint16_t* lib, int64_t N, int E, const float* row_bias, const float* par, int K, const float* cst,
                    const float* lse, float* part, int64_t part_floats, float* w, float* s1, float* s2, int blocks, void* stream);

/* CH, the rows of one chunk of coati_gmm_mstep.  Host only; it never changes within a build (the summation order hangs on it). */
int coati_gmm_chunk(void);

/* R, the ranges that the chunks of N rows are grouped into: min(ceil(N / CH), 512).  Host arithmetic only; negative on a bad N. */
int64_t coati_gmm_ranges(int64_t N);

/* The floats that part needs: R K (2 E + 1).  Host arithmetic only, no device call; negative on bad arguments (the limits above). */
int64_t coati_gmm_part_floats(int64_t N, int E, int K);

#ifdef __cplusplus
}
#endif

#endif /* COATI_GMM_H */
