/*
 * coati_pq.h -- product-quantised search over an embedding library held in device memory (csrc/pq.hip of libcoati_hip.so): every row
 * as one code byte per 8 dimensions, an encoder, and a streaming top-k over the codes with the code books in LDS.
 *
 * A seventeenth header of the same library and the same conventions as coati_hip.h (which it includes): every function returns 0 or a
 * negative code with a message in coati_last_error(), null pointers and out-of-range arguments are refused before any HIP call, all
 * pointers are DEVICE pointers owned by the caller (PyTorch), `stream` is a hipStream_t passed as void*.  coati_hip.h and
 * COATI_ABI_VERSION are unchanged by it.
 *
 * The reference has no counterpart.
 *
 * Storage: M = E / 8 sub-spaces; codebook [M][256][8] bf16, entry e of sub-space m being 8 values for dimensions 8 m .. 8 m + 7;
 * codes [N][M] uint8, codes[n][m] naming the entry that stands for those dimensions of row n.  The reconstructed row x_hat[n] [E] bf16
 * is the concatenation of its M entries: 16 times fewer bytes than the bf16 row.  `codes` must be 4-byte aligned (coati_pq_topk reads a
 * row's codes as E / 32 dwords; M is a multiple of 4) and `codebook` 16-byte aligned, as PyTorch allocations are.
 *
 * Limits of every entry: E % 32 == 0, 32 <= E <= 256, 1 <= N < 2^31, Q >= 1.
 */
#ifndef COATI_PQ_H
#define COATI_PQ_H

#include "coati_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* codes [n, E / 8] of x [n, E] bf16 under codebook [E / 8][256][8] bf16: codes[r][m] = the entry e of sub-space m with the smallest
 *   d(e) = ((((((p0 + p1) + p2) + p3) + p4) + p5) + p6) + p7,   p_j = t_j * t_j,   t_j = x[r][8 m + j] - codebook[m][e][j],
 * every difference, product and sum rounded to f32 on its own (no fused multiply-add), and among equal distances the lowest e.
 * Inputs are finite.  One pass over x; the code book is held in LDS. */
int coati_pq_encode(const uint16_t* x, int64_t n, int E, const uint16_t* codebook, uint8_t* codes, void* stream);

/* Per query i of q [Q, E] bf16: out_score / out_row [Q, k] = the k best rows by alpha * dot(q_i, x_hat_n) + bias[n] (bias [N] f32, or
 * null for none).  The contract is coati_search_topk's (coati_search.h) in every respect -- score descending, row ascending among equal
 * scores, a row whose bias is -inf is never a result, (-inf, -1) padding, the scratch part_score (f32) / part_row (int32) [Q, S, k],
 * a result that does not depend on S -- and every returned score has the BITS coati_search_topk returns for that (query, row) on the
 * bf16 library x_hat: the same v_mfma_f32_16x16x32_bf16 k-steps in ascending order from a zero accumulator, alpha * acc + bias, a zero
 * canonicalised to +0; only the operand comes from the code book (one 16-byte LDS read per code byte) instead of from memory.
 * 1 <= k <= coati_pq_k_max(E), S >= 1, S * k <= 30720.  A workgroup holds the whole code book (512 E bytes) and its queries' lists in
 * LDS: up to 152 KiB of the CU's 160 KiB at E = 256. */
int coati_pq_topk(const uint8_t* codes, int64_t N, int E, const uint16_t* codebook, const float* bias, const uint16_t* q, int Q, int k,
                  float alpha, int S, float* part_score, int32_t* part_row, float* out_score, int64_t* out_row, void* stream);

/* The largest k coati_pq_topk takes at this E: the code book (512 E bytes), the lists of a workgroup's 16 NP queries (16 NP *
 * (k + 128) * 8 bytes; NP = 2 up to E = 128, NP = 1 above) and 16 NP * 8 + 8 bytes of counts, thresholds and flags fit 160 KiB at
 * k = 128 for every E <= 224; at E = 256 (128 KiB of code book) k = 64 fits, with 24 KiB of lists.  Host arithmetic only, no device
 * call; negative on a bad E. */
int coati_pq_k_max(int E);

/* The S a caller should pass to coati_pq_topk by default: enough workgroups to fill the device at this Q, no slice shorter than 16384
 * rows (whose code bytes are 4 times the code book its workgroup loads) unless the library is, S * k <= 30720.  Host arithmetic
 * only, no device call; negative on bad arguments. */
int coati_pq_slices(int64_t N, int E, int Q, int k);

#ifdef __cplusplus
}
#endif

#endif /* COATI_PQ_H */
