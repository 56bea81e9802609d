// Property heads on rows of embeddings (include/coati_screen.h): out = last(resnet(first(x))) for every row of a bf16 library, as one
// kernel.  The library is read once, nothing but [N, P] floats is written, and no activation ever exists in memory.
//
// head_eval_kernel<F, WAVES, NP> is head_body<F, WAVES, NP, HEAD_MODE_EVAL> of head_dev.h, where the layout is described: the body is shared with the
// input-gradient kernel (guide.hip), which runs the same forward, instruction for instruction, before its backward.
// No atomics, no workspace.
#include "../../include/coati_screen.h"
#include "head_dev.h"

template <int F, int WAVES, int NP>
__global__ __launch_bounds__(64 * WAVES) void head_eval_kernel(const bf16_t* __restrict__ x, long long ldx, long long N, int E,
                                                               const bf16_t* __restrict__ w0, const float* __restrict__ b0,
                                                               const bf16_t* __restrict__ wr, const float* __restrict__ br, int D,
                                                               const float* __restrict__ wl, const float* __restrict__ bl, int P,
                                                               float* __restrict__ out, long long ldo) {
  head_body<F, WAVES, NP, HEAD_MODE_EVAL>(x, ldx, N, E, w0, b0, wr, br, D, wl, bl, P, out, ldo, nullptr, nullptr, nullptr, 0, nullptr, 0,
                                          HeadGpOps{});
}

template <int F, int WAVES, int NP>
static void head_launch(const bf16_t* x, long long ldx, long long N, int E, const bf16_t* w0, const float* b0, const bf16_t* wr,
                        const float* br, int D, const float* wl, const float* bl, int P, float* out, long long ldo, hipStream_t s) {
  hipLaunchKernelGGL((head_eval_kernel<F, WAVES, NP>), dim3(cdiv(N, WAVES * NP * 32)), dim3(64 * WAVES), 0, s, x, ldx, N, E, w0, b0, wr, br, D,
                     wl, bl, P, out, ldo);
}

static bool head_aligned16(const void* p) { return (reinterpret_cast<unsigned long long>(p) & 15ull) == 0; }

int coati_head_eval(const uint16_t* x, int64_t ldx, int64_t N, int E, const uint16_t* w0, const float* b0, const uint16_t* wr, const float* br,
                    int D, const float* wl, const float* bl, int P, int F, float* out, int64_t ldo, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(x && w0 && b0 && wl && bl && out, "head_eval: null operand");
  COATI_CHECK_SHAPE(D >= 0 && D <= HEAD_D_MAX, "head_eval: D=%d outside 0 .. %d", D, HEAD_D_MAX);
  COATI_CHECK_ARG(D == 0 || (wr && br), "head_eval: null residual weights with D=%d", D);
  COATI_CHECK_SHAPE(E >= 32 && E <= HEAD_E_MAX && E % 32 == 0, "head_eval: E=%d is not a multiple of 32 in 32 .. %d", E, HEAD_E_MAX);
  COATI_CHECK_SHAPE(F == 64 || F == 128 || F == 256, "head_eval: F=%d is not 64, 128 or 256", F);
  COATI_CHECK_SHAPE(P >= 1 && P <= HEAD_P_MAX, "head_eval: P=%d outside 1 .. %d", P, HEAD_P_MAX);
  COATI_CHECK_SHAPE(N >= 1 && N < (1ll << 31), "head_eval: N=%lld outside 1 .. 2^31 - 1", (long long)N);
  COATI_CHECK_SHAPE(ldx >= E && ldx % 8 == 0, "head_eval: ldx=%lld must be a multiple of 8 and >= E=%d", (long long)ldx, E);
  COATI_CHECK_SHAPE(ldo >= P, "head_eval: ldo=%lld < P=%d", (long long)ldo, P);
  COATI_CHECK_ARG(head_aligned16(x) && head_aligned16(w0) && head_aligned16(b0) && head_aligned16(wr) && head_aligned16(br) && head_aligned16(wl),
                  "head_eval: x, w0, b0, wr, br and wl must start at 16-byte boundaries");
  if (F == 64)
    head_launch<64, 4, 2>(x, ldx, N, E, w0, b0, wr, br, D, wl, bl, P, out, ldo, s);
  else if (F == 128)
    head_launch<128, 4, 2>(x, ldx, N, E, w0, b0, wr, br, D, wl, bl, P, out, ldo, s);
  else
    head_launch<256, HEAD_WAVES_256, HEAD_NP_256>(x, ldx, N, E, w0, b0, wr, br, D, wl, bl, P, out, ldo, s);
  COATI_LAUNCH_CHECK("head_eval");
  return COATI_OK;
}
