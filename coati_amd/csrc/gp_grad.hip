// The gradient of a GP head's acquisition with respect to its input rows (include/coati_acq.h): mean [N, P], var [N], acq [N] and g [N, E] =
// rs * d acq / dx as one launch.  head_gp_grad_kernel<F, WAVES, NP> is head_body<F, WAVES, NP, HEAD_MODE_GPGRAD> of head_dev.h:
// coati_head_grad's forward (the ReLU decisions stay as bits in LDS), coati_head_gp's tail (which here keeps w = qs k), the acquisition and
// its two derivatives per row, one more chained bf16 product against z transposed for d acq / d phi, then coati_head_grad's backward loop over
// the transposed weights.  No activation, mask, k or d ever exists in memory; no atomics, no workspace.
//
// LDS is dynamic: the two weight buffers, qs (17 KiB), then D layers of mask words: up to 153 KiB at F = 256, D = 16.  The tile is
// coati_head_grad's choice: at F = 64 and F = 128 one 32-row panel per wave while that tile's grid still is one round of the device, two
// beyond; a panel's instruction sequence does not depend on the tile around it, so the results do not depend on that choice.
#include "../../include/coati_acq.h"
#include "head_dev.h"

template <int F, int WAVES, int NP>
__global__ __launch_bounds__(64 * WAVES) void head_gp_grad_kernel(const bf16_t* __restrict__ x, long long ldx, long long N, int E,
                                                                  const bf16_t* __restrict__ w0, const float* __restrict__ b0,
                                                                  const bf16_t* __restrict__ wr, const float* __restrict__ br, int D,
                                                                  const bf16_t* __restrict__ w0t, const bf16_t* __restrict__ wrt,
                                                                  const bf16_t* __restrict__ z, const bf16_t* __restrict__ zt,
                                                                  const float* __restrict__ zn, const float* __restrict__ alpha,
                                                                  const float* __restrict__ qs, const float* __restrict__ c, float inv2l2,
                                                                  float s2, int P, int Mp, const float* __restrict__ wm, float kappa,
                                                                  float var_add, int mode, float best, const float* __restrict__ rs,
                                                                  float* __restrict__ mean, long long ldm, float* __restrict__ var,
                                                                  float* __restrict__ acq, float* __restrict__ g, long long ldg) {
  const HeadGpOps gp = {z, zn, alpha, qs, c, inv2l2, s2, P, Mp, mean, ldm, var};   // (built here: a struct parameter would live in scratch)
  const HeadAcqOps aq = {zt, wm, kappa, var_add, best, mode, rs, acq};
  head_body<F, WAVES, NP, HEAD_MODE_GPGRAD>(x, ldx, N, E, w0, b0, wr, br, D, nullptr, nullptr, 0, nullptr, 0, w0t, wrt, nullptr, 0, g, ldg, gp,
                                            aq);
}

struct HeadGpGradArgs {
  const bf16_t* x; long long ldx, N; int E;
  const bf16_t* w0; const float* b0; const bf16_t* wr; const float* br; int D;
  const bf16_t* w0t; const bf16_t* wrt;
  const bf16_t* z; const bf16_t* zt; const float* zn; const float* alpha; const float* qs; const float* c; float inv2l2, s2; int P, Mp;
  const float* wm; float kappa, var_add; int mode; float best; const float* rs;
  float* mean; long long ldm; float* var; float* acq; float* g; long long ldg;
};

template <int F, int WAVES, int NP>
static int head_gp_grad_launch(const HeadGpGradArgs& a, hipStream_t s) {
  static bool attr_set = false;
  auto kern = head_gp_grad_kernel<F, WAVES, NP>;
  if (!attr_set) {   // (the largest D: set once)
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)head_gpgrad_lds_bytes<F, WAVES, NP>(HEAD_D_MAX));
    if (e != hipSuccess) {
      coati_set_error("head_gp_grad: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
      return COATI_EHIP;
    }
    attr_set = true;
  }
  const size_t lds = head_gpgrad_lds_bytes<F, WAVES, NP>(a.D);
  hipLaunchKernelGGL(kern, dim3(cdiv(a.N, WAVES * NP * 32)), dim3(64 * WAVES), lds, s, a.x, a.ldx, a.N, a.E, a.w0, a.b0, a.wr, a.br, a.D, a.w0t,
                     a.wrt, a.z, a.zt, a.zn, a.alpha, a.qs, a.c, a.inv2l2, a.s2, a.P, a.Mp, a.wm, a.kappa, a.var_add, a.mode, a.best, a.rs,
                     a.mean, a.ldm, a.var, a.acq, a.g, a.ldg);
  COATI_LAUNCH_CHECK("head_gp_grad");
  return COATI_OK;
}

static bool acq_aligned16(const void* p) { return (reinterpret_cast<unsigned long long>(p) & 15ull) == 0; }

// the number of CUs of the current device (asked once)
static int head_gp_grad_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
      cus = v;
    else
      cus = 256;
  }
  return cus;
}

int coati_head_gp_grad(const uint16_t* x, int64_t ldx, int64_t N, int E, const uint16_t* w0, const float* b0, const uint16_t* wr,
                       const float* br, int D, int F, const uint16_t* w0t, const uint16_t* wrt, const uint16_t* z, const uint16_t* zt,
                       const float* zn, const float* alpha, const float* qs, const float* c, float inv2l2, float s2, int P, int Mp,
                       const float* wm, float kappa, float var_add, int mode, float best, const float* rs, float* mean, int64_t ldm,
                       float* var, float* acq, float* g, int64_t ldg, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(x, "head_gp_grad: x is null");
  COATI_CHECK_ARG(w0, "head_gp_grad: w0 is null");
  COATI_CHECK_ARG(b0, "head_gp_grad: b0 is null");
  COATI_CHECK_ARG(w0t, "head_gp_grad: w0t is null");
  COATI_CHECK_ARG(z, "head_gp_grad: z is null");
  COATI_CHECK_ARG(zt, "head_gp_grad: zt is null");
  COATI_CHECK_ARG(zn, "head_gp_grad: zn is null");
  COATI_CHECK_ARG(alpha, "head_gp_grad: alpha is null");
  COATI_CHECK_ARG(qs, "head_gp_grad: qs is null");
  COATI_CHECK_ARG(c, "head_gp_grad: c is null");
  COATI_CHECK_ARG(wm, "head_gp_grad: wm is null");
  COATI_CHECK_ARG(mean, "head_gp_grad: mean is null");
  COATI_CHECK_ARG(var, "head_gp_grad: var is null");
  COATI_CHECK_ARG(acq, "head_gp_grad: acq is null");
  COATI_CHECK_ARG(g, "head_gp_grad: g is null");
  COATI_CHECK_SHAPE(D >= 0 && D <= HEAD_D_MAX, "head_gp_grad: D=%d outside 0 .. %d", D, HEAD_D_MAX);
  COATI_CHECK_ARG(D == 0 || (wr && br && wrt), "head_gp_grad: null residual weights with D=%d", D);
  COATI_CHECK_SHAPE(E >= 32 && E <= HEAD_E_MAX && E % 32 == 0, "head_gp_grad: E=%d is not a multiple of 32 in 32 .. %d", E, HEAD_E_MAX);
  COATI_CHECK_SHAPE(F == 64 || F == 128 || F == 256, "head_gp_grad: F=%d is not 64, 128 or 256", F);
  COATI_CHECK_SHAPE(P >= 1 && P <= HEAD_P_MAX, "head_gp_grad: P=%d outside 1 .. %d", P, HEAD_P_MAX);
  COATI_CHECK_SHAPE(Mp == 32 || Mp == HEAD_GP_M_MAX, "head_gp_grad: Mp=%d is not 32 or %d", Mp, HEAD_GP_M_MAX);
  COATI_CHECK_SHAPE(mode == 0 || mode == 1, "head_gp_grad: mode=%d is not 0 (linear) or 1 (expected improvement)", mode);
  COATI_CHECK_SHAPE(mode == 0 || kappa > 0.f, "head_gp_grad: kappa=%g must be positive with mode=1", (double)kappa);
  COATI_CHECK_SHAPE(N >= 1 && N < (1ll << 31), "head_gp_grad: N=%lld outside 1 .. 2^31 - 1", (long long)N);
  COATI_CHECK_SHAPE(ldx >= E && ldx % 8 == 0, "head_gp_grad: ldx=%lld must be a multiple of 8 and >= E=%d", (long long)ldx, E);
  COATI_CHECK_SHAPE(ldm >= P, "head_gp_grad: ldm=%lld < P=%d", (long long)ldm, P);
  COATI_CHECK_SHAPE(ldg >= E && ldg % 4 == 0, "head_gp_grad: ldg=%lld must be a multiple of 4 and >= E=%d", (long long)ldg, E);
  COATI_CHECK_ARG(acq_aligned16(x) && acq_aligned16(w0) && acq_aligned16(b0) && acq_aligned16(wr) && acq_aligned16(br) && acq_aligned16(w0t) &&
                      acq_aligned16(wrt) && acq_aligned16(g),
                  "head_gp_grad: x, w0, b0, wr, br, w0t, wrt and g must start at 16-byte boundaries");
  COATI_CHECK_ARG(acq_aligned16(z) && acq_aligned16(zt) && acq_aligned16(zn) && acq_aligned16(alpha) && acq_aligned16(qs),
                  "head_gp_grad: z, zt, zn, alpha and qs must start at 16-byte boundaries");
  const HeadGpGradArgs a = {x, ldx, N, E, w0, b0, wr, br, D, w0t, wrt, z, zt, zn, alpha, qs, c, inv2l2, s2, P, Mp,
                            wm, kappa, var_add, mode, best, rs, mean, ldm, var, acq, g, ldg};
  // coati_head_grad's choice: narrow while the narrow tile's grid is one round of the device (F = 64 keeps two of its workgroups per CU)
  const bool narrow = cdiv(N, 128) <= head_gp_grad_cus() * (F == 64 ? 2 : 1);
  if (F == 64)
    return narrow ? head_gp_grad_launch<64, 4, 1>(a, s) : head_gp_grad_launch<64, 4, 2>(a, s);
  if (F == 128)
    return narrow ? head_gp_grad_launch<128, 4, 1>(a, s) : head_gp_grad_launch<128, 4, 2>(a, s);
  return head_gp_grad_launch<256, HEAD_WAVES_256, HEAD_NP_256>(a, s);
}
