// The gradient of a property head with respect to its input rows (include/coati_guide.h): out = head(x) and g = d (cot . out) / dx as one
// launch.  head_grad_kernel<F, WAVES, NP> is head_body<F, WAVES, NP, HEAD_MODE_GRAD> of head_dev.h: coati_head_eval's forward, instruction for
// instruction, which also leaves the ReLU decisions as bits in LDS, then the backward through the same chunked, register-chained product
// loop over the transposed weights.  No activation, mask or d ever exists in memory; no atomics, no workspace.
//
// LDS is dynamic (the two weight buffers, then D layers of mask words: up to 136 KiB at F = 256, D = 16).  At F = 64 and F = 128 the
// launcher picks a narrower tile (one 32-row panel per wave, not two) while that tile's grid still is one round of the device; a 32-row
// panel's instruction sequence does not depend on the tile around it, so the results do not depend on that choice.
#include "../../include/coati_guide.h"
#include "head_dev.h"

template <int F, int WAVES, int NP>
__global__ __launch_bounds__(64 * WAVES) void head_grad_kernel(const bf16_t* __restrict__ x, long long ldx, long long N, int E,
                                                               const bf16_t* __restrict__ w0, const float* __restrict__ b0,
                                                               const bf16_t* __restrict__ wr, const float* __restrict__ br, int D,
                                                               const float* __restrict__ wl, const float* __restrict__ bl, int P,
                                                               const bf16_t* __restrict__ w0t, const bf16_t* __restrict__ wrt,
                                                               const float* __restrict__ cot, long long ldc, float* __restrict__ out,
                                                               long long ldo, float* __restrict__ g, long long ldg) {
  head_body<F, WAVES, NP, HEAD_MODE_GRAD>(x, ldx, N, E, w0, b0, wr, br, D, wl, bl, P, out, ldo, w0t, wrt, cot, ldc, g, ldg, HeadGpOps{});
}

struct HeadGradArgs {
  const bf16_t* x; long long ldx, N; int E;
  const bf16_t* w0; const float* b0; const bf16_t* wr; const float* br; int D;
  const float* wl; const float* bl; int P;
  const bf16_t* w0t; const bf16_t* wrt; const float* cot; long long ldc;
  float* out; long long ldo; float* g; long long ldg;
};

template <int F, int WAVES, int NP>
static int head_grad_launch(const HeadGradArgs& a, hipStream_t s) {
  static bool attr_set = false;
  auto kern = head_grad_kernel<F, WAVES, NP>;
  if (!attr_set) {   // (the largest D: set once)
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)head_grad_lds_bytes<F, WAVES, NP>(HEAD_D_MAX));
    if (e != hipSuccess) {
      coati_set_error("head_grad: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
      return COATI_EHIP;
    }
    attr_set = true;
  }
  const size_t lds = head_grad_lds_bytes<F, WAVES, NP>(a.D);
  hipLaunchKernelGGL(kern, dim3(cdiv(a.N, WAVES * NP * 32)), dim3(64 * WAVES), lds, s, a.x, a.ldx, a.N, a.E,
                     a.w0, a.b0, a.wr, a.br, a.D, a.wl, a.bl, a.P, a.w0t, a.wrt, a.cot, a.ldc, a.out, a.ldo, a.g, a.ldg);
  COATI_LAUNCH_CHECK("head_grad");
  return COATI_OK;
}

static bool grad_aligned16(const void* p) { return (reinterpret_cast<unsigned long long>(p) & 15ull) == 0; }

// the number of CUs of the current device (asked once)
static int head_grad_cus() {
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

int coati_head_grad(const uint16_t* x, int64_t ldx, int64_t N, int E, const uint16_t* w0, const float* b0, const uint16_t* wr, const float* br,
                    int D, const float* wl, const float* bl, int P, int F, const uint16_t* w0t, const uint16_t* wrt, const float* cot,
                    int64_t ldc, float* out, int64_t ldo, float* g, int64_t ldg, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(x && w0 && b0 && wl && bl && w0t && cot && out && g, "head_grad: null operand");
  COATI_CHECK_SHAPE(D >= 0 && D <= HEAD_D_MAX, "head_grad: D=%d outside 0 .. %d", D, HEAD_D_MAX);
  COATI_CHECK_ARG(D == 0 || (wr && br && wrt), "head_grad: null residual weights with D=%d", D);
  COATI_CHECK_SHAPE(E >= 32 && E <= HEAD_E_MAX && E % 32 == 0, "head_grad: E=%d is not a multiple of 32 in 32 .. %d", E, HEAD_E_MAX);
  COATI_CHECK_SHAPE(F == 64 || F == 128 || F == 256, "head_grad: F=%d is not 64, 128 or 256", F);
  COATI_CHECK_SHAPE(P >= 1 && P <= HEAD_P_MAX, "head_grad: P=%d outside 1 .. %d", P, HEAD_P_MAX);
  COATI_CHECK_SHAPE(N >= 1 && N < (1ll << 31), "head_grad: N=%lld outside 1 .. 2^31 - 1", (long long)N);
  COATI_CHECK_SHAPE(ldx >= E && ldx % 8 == 0, "head_grad: ldx=%lld must be a multiple of 8 and >= E=%d", (long long)ldx, E);
  COATI_CHECK_SHAPE(ldo >= P, "head_grad: ldo=%lld < P=%d", (long long)ldo, P);
  COATI_CHECK_SHAPE(ldc >= P, "head_grad: ldc=%lld < P=%d", (long long)ldc, P);
  COATI_CHECK_SHAPE(ldg >= E && ldg % 4 == 0, "head_grad: ldg=%lld must be a multiple of 4 and >= E=%d", (long long)ldg, E);
  COATI_CHECK_ARG(grad_aligned16(x) && grad_aligned16(w0) && grad_aligned16(b0) && grad_aligned16(wr) && grad_aligned16(br) && grad_aligned16(wl) &&
                      grad_aligned16(w0t) && grad_aligned16(wrt) && grad_aligned16(g),
                  "head_grad: x, w0, b0, wr, br, wl, w0t, wrt and g must start at 16-byte boundaries");
  const HeadGradArgs a = {x, ldx, N, E, w0, b0, wr, br, D, wl, bl, P, w0t, wrt, cot, ldc, out, ldo, g, ldg};
#ifdef HEAD_GRAD_TILE   // probe builds: 1 = the narrow tile at every N, 2 = the wide one ("Guided optimisation")
  const bool narrow = HEAD_GRAD_TILE == 1;
#else
  // narrow while the narrow tile's grid is one round of the device: F = 64 keeps two of its workgroups per CU, F = 128 one
  const bool narrow = cdiv(N, 128) <= head_grad_cus() * (F == 64 ? 2 : 1);
#endif
  if (F == 64)
    return narrow ? head_grad_launch<64, 4, 1>(a, s) : head_grad_launch<64, 4, 2>(a, s);
  if (F == 128)
    return narrow ? head_grad_launch<128, 4, 1>(a, s) : head_grad_launch<128, 4, 2>(a, s);
  // F = 256 has one tile: its wide tile already is one panel per wave, and two waves per workgroup would stage 64 registers of weights per
  // thread next to the 128 of the stream
  return head_grad_launch<256, HEAD_WAVES_256, HEAD_NP_256>(a, s);
}
