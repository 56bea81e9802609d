/*
 * coati_gnn_ops.h -- the point encoder's edge-level, backward and device-side-row-count kernels one by one (csrc/gnn.hip,
 * csrc/gemm_rb16.hip, csrc/gemm.hip of libcoati_hip.so), so that each can be tested against plain maths on its own.
 *
 * A thirteenth header of the same library and the same conventions as coati_hip.h (which it includes): every function returns 0 or a
 * negative code with a message in coati_last_error(), null pointers and out-of-range arguments are refused before any HIP call, all
 * pointers are DEVICE pointers owned by the caller (PyTorch) unless said otherwise, `stream` is a hipStream_t passed as void*.
 * coati_hip.h and COATI_ABI_VERSION are unchanged by it.  Nothing on the engine's path goes through these entries: they are thin
 * wrappers of the launchers the engine calls itself (csrc/kernels.h), argument for argument.
 *
 * The compacted edge list is what coati_gnn_compact emits: edges in receiver-major order, seg [BA + 1] the receivers' segments,
 * e_bj / e_bk [E] the receiver / sender node row of an edge, e_rev [E] the index of the opposite edge, e_d2 / e_w [E] the squared
 * distance and the cutoff weight, n_edges[0] = E.  bf16 tensors are uint16_t.
 */
#ifndef COATI_GNN_OPS_H
#define COATI_GNN_OPS_H

#include "coati_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The forward edge path as one launch, H = 256 only (any other H is refused):
 *   e1[e] = SiLU(P[bj, :H] + P[bk, H:] + e_d2[e] w1c + b1),  s2[e] = e1[e] W3^T + b3 (e1 as stored, bf16),
 *   mi[bj] = sum over the receiver's segment of SiLU(s2[e]) e_w[e] (s2 as stored; zero for a receiver without edges).
 * P [BA, ldp] bf16, w1c[c] = w1c[c * w1c_stride], W3 [H, ldw] bf16, e1 / s2 [E, H] bf16, mi [BA, ldmi] bf16. */
int coati_gnn_edge_fwd_fused(const uint16_t* P, int64_t ldp, const int32_t* seg, const int32_t* e_bk, const float* e_d2, const float* e_w,
                             const float* w1c, int64_t w1c_stride, const float* b1, const uint16_t* W3, int64_t ldw, const float* b3,
                             uint16_t* e1, uint16_t* s2, uint16_t* mi, int64_t ldmi, int BA, int H, void* stream);

/* ds2[e] = dmi[receiver(e)] e_w[e] SiLU'(s2[e]);  dmi [BA, lddmi], s2 / ds2 [E, H] bf16; H % 4 == 0 */
int coati_gnn_edge_reduce_bwd(const uint16_t* dmi, int64_t lddmi, const uint16_t* s2, const int32_t* seg, const float* e_w, uint16_t* ds2,
                              int BA, int H, void* stream);

/* dP[bj, :H] = sum over the receiver's segment of dpre[e];  dP[bj, H:2H] = the same sum over the rows e_rev[e];
 * dw1c[c * dw1c_stride] += sum over all edges of dpre[e, c] e_d2[e];  db1[c] += sum over all edges of dpre[e, c].
 * dpre [E, H] bf16, dP [BA, lddp] bf16 (every row is written), dw1c / db1 f32, accumulated with atomics; H % 4 == 0 */
int coati_gnn_edge_pre_bwd(const uint16_t* dpre, const int32_t* seg, const int32_t* e_rev, const float* e_d2, uint16_t* dP, int64_t lddp,
                           float* dw1c, int64_t dw1c_stride, float* db1, int BA, int H, void* stream);

/* residual = True: v = u32[row] + W3c[:, ix] + W3c[:, iy] (the hot one-hot columns of the atom, W3c[c, i] = W3c[c * ldw + i]; an index
 * of -1 adds nothing), upre = bf16(v), t16 = bf16(SiLU(v));  u32 [BA, H] f32, lut_ix / lut_iy [120] int32 */
int coati_gnn_node_res_silu(const float* u32, const int64_t* atoms, const int32_t* lut_ix, const int32_t* lut_iy, const float* W3c,
                            int64_t ldw, uint16_t* upre, uint16_t* t16, int BA, int H, void* stream);

/* dW[c * ldw + i] += sum over the atoms whose one-hot has bit i of du[atom, c];  du [BA, H] bf16 */
int coati_gnn_onehot_wgrad(const int64_t* atoms, const int32_t* lut_ix, const int32_t* lut_iy, const uint16_t* du, float* dW, int64_t ldw,
                           int BA, int H, void* stream);

/* The embedding's backward.  One-hot form: dW [H, 28] += the per-bit sums of de [BA, H] f32, db [H] += the sum over all atoms.
 * lut_ix, lut_iy and db all null: the table form, dW [84, H] += de summed per atomic number (clamped to 0 .. 83). */
int coati_gnn_embed_bwd(const int64_t* atoms, const int32_t* lut_ix, const int32_t* lut_iy, const float* de, float* dW, float* db, int BA,
                        int H, void* stream);

/* hp[b] = sum_a o[b, a] mask[b, a] / max(sum_a mask[b, a], 1);  o [B, A, H] f32, mask [B, A] f32, hp [B, H] f32 */
int coati_gnn_readout(const float* o, const float* mask, float* hp, int B, int A, int H, void* stream);
/* dout[b, a] = bf16(dhp[b] / max(sum_a mask[b, a], 1) * mask[b, a]);  dout [B, A, H] bf16 */
int coati_gnn_readout_bwd(const float* dhp, const float* mask, uint16_t* dout, int B, int A, int H, void* stream);

/* C [rows, N] bf16 = A [rows, K] bf16 times B [N, K]^T with rows = m_dev[0] read on the DEVICE (<= M; M sizes the grid only).
 * epi = 0 (EPI_BF16): + bias.  epi = 10 (EPI_EDGE_DPRE): times SiLU'(P[bj, :H] + P[bk, H:] + d2[row] w1c + b1) of the row's edge
 * (N == H; e_bj / e_bk the compacted list, or both null for the dense grid of natom atoms).  No other epilogue.  Rows from m_dev[0]
 * on are not written.  *resident (HOST int, required) = 1 when the weight-resident persistent kernel took the shape, else 0. */
int coati_gemm_rows_dev(const int32_t* m_dev, const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, int M, int N, int K,
                        uint16_t* C, int64_t ldc, const float* bias, int epi, const uint16_t* P, int64_t ldp, const float* d2,
                        const float* w1c, int64_t w1c_stride, const float* b1, int natom, int H, const int32_t* e_bj,
                        const int32_t* e_bk, int32_t* resident, void* stream);

/* dW [N, ldw] f32 += A[:rows]^T B[:rows], dbias [N] += colsum(A[:rows]) (null: none), rows = m_dev[0] read on the device (<= M) */
int coati_wgrad_rows_dev(const int32_t* m_dev, const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, int M, int N, int K,
                         float* dW, int64_t ldw, float* dbias, void* stream);

/* Several weight gradients of M rows each in one launch, every problem's 128 x 128 tiles repeated over n_splits slices of M and added with
 * fp32 atomics (the point encoder's node-level Linears).  The arrays of n_problems entries live on the HOST; dbias[i] may be null.  The
 * table is built on the host and uploaded into `workspace` (device, coati_wgrad_split_workspace_bytes at least). */
int64_t coati_wgrad_split_workspace_bytes(int n_problems, const int* N, const int* K, int n_splits);
int coati_wgrad_split(int n_problems, const uint16_t* const* A, const int64_t* lda, const uint16_t* const* B, const int64_t* ldb, int M,
                      const int* N, const int* K, float* const* dW, const int64_t* ldw, float* const* dbias, int n_splits,
                      void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* COATI_GNN_OPS_H */
