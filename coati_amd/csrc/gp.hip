// A Gaussian-process head on inducing points, on top of the property head's features (include/coati_gp.h): mean [N, P] and var [N] of every
// row of a bf16 library as one launch.  head_gp_kernel<F, WAVES, NP> is head_body<F, WAVES, NP, HEAD_MODE_GP> of head_dev.h: coati_head_eval's
// forward, instruction for instruction (with wl given it also writes coati_head_eval's out), then the GP tail on the stream the forward
// leaves in registers: one more chained bf16 product against the inducing points, Mp exponentials per row, a dot product per output and a
// quadratic form on the f32 matrix cores.  The library is read once, no [N, F] feature matrix exists in memory; no atomics, no workspace.
#include "../../include/coati_gp.h"
#include "head_dev.h"

template <int F, int WAVES, int NP>
__global__ __launch_bounds__(64 * WAVES) void head_gp_kernel(const bf16_t* __restrict__ x, long long ldx, long long N, int E,
                                                             const bf16_t* __restrict__ w0, const float* __restrict__ b0,
                                                             const bf16_t* __restrict__ wr, const float* __restrict__ br, int D,
                                                             const float* __restrict__ wl, const float* __restrict__ bl, int P_lin,
                                                             float* __restrict__ out, long long ldo, const bf16_t* __restrict__ z,
                                                             const float* __restrict__ zn, const float* __restrict__ alpha,
                                                             const float* __restrict__ q, const float* __restrict__ c, float inv2l2, float s2,
                                                             int P, int Mp, float* __restrict__ mean, long long ldm,
                                                             float* __restrict__ var) {
  const HeadGpOps gp = {z, zn, alpha, q, c, inv2l2, s2, P, Mp, mean, ldm, var};   // (built here: a struct parameter would live in scratch)
  head_body<F, WAVES, NP, HEAD_MODE_GP>(x, ldx, N, E, w0, b0, wr, br, D, wl, bl, P_lin, out, ldo, nullptr, nullptr, nullptr, 0, nullptr, 0, gp);
}

template <int F, int WAVES, int NP>
static void head_gp_launch(const bf16_t* x, long long ldx, long long N, int E, const bf16_t* w0, const float* b0, const bf16_t* wr,
                           const float* br, int D, const float* wl, const float* bl, int P_lin, float* out, long long ldo,
                           const HeadGpOps& gp, hipStream_t s) {
  hipLaunchKernelGGL((head_gp_kernel<F, WAVES, NP>), dim3(cdiv(N, WAVES * NP * 32)), dim3(64 * WAVES), 0, s, x, ldx, N, E, w0, b0, wr, br, D,
                     wl, bl, P_lin, out, ldo, gp.z, gp.zn, gp.alpha, gp.q, gp.c, gp.inv2l2, gp.s2, gp.P, gp.Mp, gp.mean, gp.ldm, gp.var);
}

static bool gp_aligned16(const void* p) { return (reinterpret_cast<unsigned long long>(p) & 15ull) == 0; }

int coati_head_gp(const uint16_t* x, int64_t ldx, int64_t N, int E, const uint16_t* w0, const float* b0, const uint16_t* wr, const float* br,
                  int D, int F, const float* wl, const float* bl, int P_lin, float* out, int64_t ldo, const uint16_t* z, const float* zn,
                  const float* alpha, const float* q, const float* c, float inv2l2, float s2, int P, int Mp, float* mean, int64_t ldm,
                  float* var, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(x, "head_gp: x is null");
  COATI_CHECK_ARG(w0, "head_gp: w0 is null");
  COATI_CHECK_ARG(b0, "head_gp: b0 is null");
  COATI_CHECK_ARG(z, "head_gp: z is null");
  COATI_CHECK_ARG(zn, "head_gp: zn is null");
  COATI_CHECK_ARG(alpha, "head_gp: alpha is null");
  COATI_CHECK_ARG(q, "head_gp: q is null");
  COATI_CHECK_ARG(c, "head_gp: c is null");
  COATI_CHECK_ARG(mean, "head_gp: mean is null");
  COATI_CHECK_ARG(var, "head_gp: var is null");
  COATI_CHECK_SHAPE(D >= 0 && D <= HEAD_D_MAX, "head_gp: D=%d outside 0 .. %d", D, HEAD_D_MAX);
  COATI_CHECK_ARG(D == 0 || (wr && br), "head_gp: null residual weights with D=%d", D);
  COATI_CHECK_SHAPE(E >= 32 && E <= HEAD_E_MAX && E % 32 == 0, "head_gp: E=%d is not a multiple of 32 in 32 .. %d", E, HEAD_E_MAX);
  COATI_CHECK_SHAPE(F == 64 || F == 128 || F == 256, "head_gp: F=%d is not 64, 128 or 256", F);
  COATI_CHECK_SHAPE(P >= 1 && P <= HEAD_P_MAX, "head_gp: P=%d outside 1 .. %d", P, HEAD_P_MAX);
  COATI_CHECK_SHAPE(Mp == 32 || Mp == HEAD_GP_M_MAX, "head_gp: Mp=%d is not 32 or %d", Mp, HEAD_GP_M_MAX);
  COATI_CHECK_SHAPE(N >= 1 && N < (1ll << 31), "head_gp: N=%lld outside 1 .. 2^31 - 1", (long long)N);
  COATI_CHECK_SHAPE(ldx >= E && ldx % 8 == 0, "head_gp: ldx=%lld must be a multiple of 8 and >= E=%d", (long long)ldx, E);
  COATI_CHECK_SHAPE(ldm >= P, "head_gp: ldm=%lld < P=%d", (long long)ldm, P);
  if (wl) {   // the linear last layer of coati_head_eval, in the same pass
    COATI_CHECK_ARG(bl, "head_gp: wl given with bl null");
    COATI_CHECK_ARG(out, "head_gp: wl given with out null");
    COATI_CHECK_SHAPE(P_lin >= 1 && P_lin <= HEAD_P_MAX, "head_gp: P_lin=%d outside 1 .. %d", P_lin, HEAD_P_MAX);
    COATI_CHECK_SHAPE(ldo >= P_lin, "head_gp: ldo=%lld < P_lin=%d", (long long)ldo, P_lin);
  }
  COATI_CHECK_ARG(gp_aligned16(x) && gp_aligned16(w0) && gp_aligned16(b0) && gp_aligned16(wr) && gp_aligned16(br) && gp_aligned16(wl),
                  "head_gp: x, w0, b0, wr, br and wl must start at 16-byte boundaries");
  COATI_CHECK_ARG(gp_aligned16(z) && gp_aligned16(zn) && gp_aligned16(alpha) && gp_aligned16(q),
                  "head_gp: z, zn, alpha and q must start at 16-byte boundaries");
  const HeadGpOps gp = {z, zn, alpha, q, c, inv2l2, s2, P, Mp, mean, ldm, var};
  const int pl = wl ? P_lin : 0;   // no wl: the last layer's loop runs zero times
  if (F == 64)
    head_gp_launch<64, 4, 2>(x, ldx, N, E, w0, b0, wr, br, D, wl, bl, pl, out, ldo, gp, s);
  else if (F == 128)
    head_gp_launch<128, 4, 2>(x, ldx, N, E, w0, b0, wr, br, D, wl, bl, pl, out, ldo, gp, s);
  else
    head_gp_launch<256, HEAD_WAVES_256, HEAD_NP_256>(x, ldx, N, E, w0, b0, wr, br, D, wl, bl, pl, out, ldo, gp, s);
  COATI_LAUNCH_CHECK("head_gp");
  return COATI_OK;
}
