/*
 * coati_acq.h -- the gradient of a GP head's acquisition with respect to its input rows (csrc/gp_grad.hip of libcoati_hip.so): what an
 * uncertainty-aware optimiser in the embedding space climbs.
 *
 * A ninth header of the same library and the same conventions as coati_hip.h (which it includes): every function returns 0 or a negative
 * code with a message in coati_last_error(), null pointers and out-of-range arguments are refused before any HIP call, all pointers are
 * DEVICE pointers owned by the caller (PyTorch), `stream` is a hipStream_t passed as void*.  coati_hip.h, coati_gp.h, the other headers and
 * COATI_ABI_VERSION are unchanged by it.
 *
 * The extractor is coati_screen.h's FC-ResNet, the GP coati_gp.h's.  One launch carries a tile of rows through the forward (recording the
 * ReLU decisions as bits), the GP, the acquisition, and back through the GP and the layers: no activation, mask, kernel vector or
 * intermediate gradient in memory, no workspace, no atomics.
 *
 * Arithmetic (GPHead.reference_acq_grad in coati_amd/models/regression/gp_head.py restates it in torch, rounding points included):
 *   phi, d2_j, k_j, mean_p exactly as coati_head_gp;  w = qs k,  v = max(0, s2 - k . w)  with qs the SYMMETRIC part of q, f32((q + q^T) / 2)
 *       formed by the caller: k q k = k qs k, and dv / dk = -2 qs k holds for qs only.  mean is coati_head_gp's bit for bit; var is where
 *       qs == q
 *   sd     = sqrt(v + var_add),   m = sum_p wm[p] mean_p
 *   mode 0 a = m + kappa sd                               A = 1,       B = kappa / (2 sd)
 *   mode 1 mu = m - best, s = kappa sd, u = mu / s        a = mu Phi(u) + s phi(u),  A = Phi(u),  B = phi(u) kappa / (2 sd)     (kappa > 0)
 *          where s == 0: a = max(mu, 0), A = [mu > 0], B = 0.     Phi(u) = (1 + erff(u / sqrt 2)) / 2, phi the normal density
 *   B = 0  in both modes where v == 0 (clamped) or v + var_add <= 1e-6 s2: the f32 cancellation in s2 - k . w has no digits left there
 *   t_j    = rs (A sum_p wm[p] alpha[p, j] - 2 B w_j) k_j          f32;  rs the row's scale, 1 when rs is null
 *   tb     = rb(t),   S = sum_j tb_j                               f32 over the rounded values
 *   dphi_f = 2 inv2l2 (sum_j tb_j z[j, f] - phi_f S)               bf16 operands, f32 accumulation (matrix cores)
 *   d = dphi;  d = d + rb(m[l] (.) d) . wr[l], l = D - 1 .. 0;  g = rb(d) . w0      exactly the backward of coati_head_grad
 * The rounding h_D -> phi is passed straight through.  g is the gradient of rs * a with respect to the row as the kernel reads it (the
 * prepared bf16 row).  What NaN / inf inputs do is unspecified.
 */
#ifndef COATI_ACQ_H
#define COATI_ACQ_H

#include "coati_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mean[n, p], var[n], acq[n] and g[n, e] for n < N, p < P, e < E.  x, ldx, N, E, w0, b0, wr, br, D, F: as in coati_head_eval
 * (coati_screen.h);  w0t [E, F], wrt [D, F, F] (null iff D == 0), g, ldg: as in coati_head_grad (coati_guide.h);  z, zn, alpha, c, inv2l2,
 * s2, P, Mp, mean, ldm, var: as in coati_head_gp (coati_gp.h);  the same domains and alignments.
 * zt [F, Mp] bf16 is z transposed;  qs [Mp, Mp] f32 the symmetric part of q;  both start at 16-byte boundaries.  A padded inducing point
 * carries zero alpha and a zero row and column of qs and then contributes exactly nothing to any output.
 * wm [P] f32 weights on the means;  kappa, var_add (0 or the noise variance), best: f32 scalars;  mode 0 or 1, mode 1 needs kappa > 0.
 * rs [N] f32 scales the gradient (not acq) per row, or null.  acq f32 [N].
 * Columns P .. ldm-1 of mean, columns E .. ldg-1 of g and rows >= N are not written.  g must not overlap x (not checked). */
int coati_head_gp_grad(const uint16_t* x, int64_t ldx, int64_t N, int E, const uint16_t* w0, const float* b0,
                       const uint16_t* wr, const float* br, int D, int F,
                       const uint16_t* w0t, const uint16_t* wrt,
                       const uint16_t* z, const uint16_t* zt, const float* zn, const float* alpha, const float* qs, const float* c,
                       float inv2l2, float s2, int P, int Mp,
                       const float* wm, float kappa, float var_add, int mode, float best, const float* rs,
                       float* mean, int64_t ldm, float* var, float* acq, float* g, int64_t ldg, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* COATI_ACQ_H */
