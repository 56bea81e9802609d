// Library density (include/coati_gmm.h): the two passes of an EM iteration of a mixture of K diagonal Gaussians over bf16 library rows.
// No [N, K] matrix, no atomics; what is written is a function of the operands alone -- not of the grid, the stream or the run.
//
// The logit of a row under a component is one product at width 2E, [x | x^2] against the component's parameter row, in f32 throughout:
// v_mfma_f32_16x16x4_f32, library rows its M side, components its N side.  Lane l holds A[row l & 15][k = l >> 4] and
// B[k = l >> 4][component l & 15], one f32 each; the result map (column = lane & 15, row = 4 (lane >> 4) + register) gives a lane four rows
// of ONE component per panel of 16, as in cluster_assign_kernel.  The reduction index may be permuted freely as long as A and B agree: step
// (q, j), lane group g stands for dimension 32 q + 8 g + j, so that a lane's A values of one q are 16 contiguous bytes of its row (bf16,
// kept packed in registers and widened by a shift in front of the MFMA; the square is one v_mul_f32, exact) and its B values two 16-byte
// LDS reads per half.
//
// gmm_panel_logits is the one device function that makes logits: for panel p it walks the KS = E / 32 stages (q ascending) of 16
// components x 32 dimensions x {linear, quadratic} = 4 KiB, double-buffered through LDS in fragment order ([half][j / 4][lane] 16-B slots),
// stage u + 1 fetched into a register before stage u's MFMAs and written to the other image after them, one barrier per stage; the last
// stage fetches the first one of the panel the caller names next.  The linear and the quadratic half have an accumulator each (two
// independent chains per slab: the instruction's 40-cycle dependent latency against its 32-cycle issue), added once at the end.  KS is a
// template argument, so the register arrays are indexed by constants only and the sweep is straight-line code.
//
// gmm_estep_kernel, 4 waves, a workgroup takes tiles of 128 rows in turn: a wave's 2 slabs of 16 rows stay in registers (2 x KS x 4
// VGPRs, 128 at E = 512) while the panels pass in ascending order.  A lane keeps, for each of its 8 result rows, a running (max, scaled
// sum) and a running (best logit, component).  Both maxima start at finite values / are replaced on a strict `>`, a column >= K is skipped
// and a logit is clamped to >= -FLT_MAX, so no -inf - -inf can occur, not even in a lane that met no component (K < 16).  The 16 lanes of
// a row meet once after the sweep (4 xor steps): larger maximum + the other's sum scaled down; larger logit, then lower component.
// Rows >= N of the last tile are read at row N - 1 and never stored.
//
// gmm_mstep_kernel, 4 waves, a work item is (range of chunks, panel): per chunk of 64 rows a wave loads its slab of 16 rows once, keeps
// it as the A operand of the logits and writes it to an LDS row tile (bf16, pitch 2E + 16 bytes); r = exp(logit - lse) (0 for rows
// >= N, excluded rows and columns >= K) goes to LDS in the result map's own order, which IS the A operand of the second product: with
// step t of a slab standing for rows 4 g + t, register t of lane (g, column) is A[component][k = g].  The waves then share the dimensions:
// wave w takes the 16-wide blocks w, w + 4, ... and runs s1 += r^T x, s2 += r^T x^2 over the 4 slabs x 4 steps in ascending order (B read
// as bf16 from the row tile); wave 3 adds w += r^T 1.  The accumulators live in registers over the whole range, then one block of `part`
// is written; gmm_finish_kernel adds the ranges in ascending order.
#include "../../include/coati_gmm.h"
#include "kernels.h"

#include <cfloat>

#define GM_E_MAX 512
#define GM_K_MAX 256
#define GM_CH 64          // rows of an M-step chunk
#define GM_RANGES 512     // the most ranges of an M-step
#define GM_SL 2           // slabs of 16 rows per wave in the E-step
#define GM_ESTEP_GRID 1024

typedef float gmm_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned gmm_u32x4 __attribute__((ext_vector_type(4)));   // 16 bytes of bf16

// Thread tid's 16-B piece of stage (panel p, q): tid = [half h][g >> 1][component 0 .. 15][g & 1][j / 4] -- four threads read 64
// contiguous bytes -- and its slot [h][j / 4][16 g + component] of the LDS image, from which lane (g, component) reads its fragment.
template <int KS>
__device__ __forceinline__ gmm_f32x4 gmm_fetch(const float* __restrict__ par, int K, int p, int q, int tid) {
  const int jj = tid & 1, g = ((tid >> 1) & 1) | ((tid >> 5) & 2), col = (tid >> 2) & 15, h = tid >> 7;
  const int k = min(16 * p + col, K - 1);   // a column >= K reads component K - 1 (inside the allocation); its logit is never used
  return *reinterpret_cast<const gmm_f32x4*>(par + (long long)k * (64 * KS) + h * (32 * KS) + 32 * q + 8 * g + 4 * jj);
}
__device__ __forceinline__ void gmm_stash(gmm_f32x4 v, gmm_f32x4* image, int tid) {
  const int jj = tid & 1, g = ((tid >> 1) & 1) | ((tid >> 5) & 2), col = (tid >> 2) & 15, h = tid >> 7;
  image[h * 128 + jj * 64 + g * 16 + col] = v;
}

// lin[sl][r] + sq[sl][r] = sum_d (x par[k, d]) + sum_d (x^2 par[k, E + d]) of rows 4 g + r of slab sl under component k = 16 p + (lane & 15).
// On entry image `buf` of `stage` holds stage (p, 0) behind a barrier; on exit image `buf` holds stage (p_next, 0) behind a barrier
// (p_next < 0: nothing).  p, p_next are workgroup-uniform: every barrier is met by all 256 threads.
template <int KS, int SL>
__device__ __forceinline__ void gmm_panel_logits(const gmm_u32x4 (&a)[SL][KS], const float* __restrict__ par, int K, int p, int p_next,
                                                 gmm_f32x4* stage, int& buf, int tid, int lane, gmm_f32x4 (&lin)[SL], gmm_f32x4 (&sq)[SL]) {
#pragma unroll
  for (int sl = 0; sl < SL; ++sl) {
    lin[sl] = gmm_f32x4{0.f, 0.f, 0.f, 0.f};
    sq[sl] = gmm_f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int q = 0; q < KS; ++q) {
    const bool more = q + 1 < KS || p_next >= 0;
    gmm_f32x4 nx = gmm_f32x4{0.f, 0.f, 0.f, 0.f};
    if (more) nx = gmm_fetch<KS>(par, K, q + 1 < KS ? p : p_next, q + 1 < KS ? q + 1 : 0, tid);
    const gmm_f32x4* im = stage + buf * 256;
    const gmm_f32x4 b1[2] = {im[lane], im[64 + lane]};
    const gmm_f32x4 b2[2] = {im[128 + lane], im[192 + lane]};
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int sl = 0; sl < SL; ++sl) {
        unsigned w = a[sl][q][j >> 1];
        asm volatile("" : "+v"(w));   // x and x^2 are made here, per panel: hoisted out of the caller's panel loop they would triple the registers
        const float x = __uint_as_float((j & 1) ? (w & 0xffff0000u) : (w << 16));
        lin[sl] = __builtin_amdgcn_mfma_f32_16x16x4f32(x, b1[j >> 2][j & 3], lin[sl], 0, 0, 0);
        sq[sl] = __builtin_amdgcn_mfma_f32_16x16x4f32(x * x, b2[j >> 2][j & 3], sq[sl], 0, 0, 0);
      }
    if (more) gmm_stash(nx, stage + (buf ^ 1) * 256, tid);   // (that image's readers were the stage before this one, behind its barrier)
    __syncthreads();
    buf ^= 1;
  }
}

// the logit as both kernels take it: the two halves, then cst, never below -FLT_MAX
__device__ __forceinline__ float gmm_logit(float lin, float sq, float c) { return fmaxf((lin + sq) + c, -FLT_MAX); }

template <int KS>
__global__ __launch_bounds__(256, 2) void gmm_estep_kernel(const bf16_t* __restrict__ lib, long long N, const float* __restrict__ row_bias,
                                                           const float* __restrict__ par, int K, const float* __restrict__ cst,
                                                           float* __restrict__ lse, int* __restrict__ assign) {
  __shared__ gmm_f32x4 stage[512];   // two images of 4 KiB
  constexpr int SL = GM_SL, ROWS = 64 * SL, E = 32 * KS;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), col = lane & 15, g = lane >> 4;
  const int panels = (K + 15) >> 4;
  const long long rtiles = (N + ROWS - 1) / ROWS;
  int buf = 0;
  if ((long long)blockIdx.x < rtiles) gmm_stash(gmm_fetch<KS>(par, K, 0, 0, tid), stage, tid);
  __syncthreads();

  for (long long rt = blockIdx.x; rt < rtiles; rt += gridDim.x) {
    // the wave's slabs: rows r0 + 16 sl + (0 .. 15); a[sl][q] = the row's dimensions 32 q + 8 g + (0 .. 7)
    const long long r0 = rt * ROWS + (long long)wave * 16 * SL;
    gmm_u32x4 a[SL][KS];
#pragma unroll
    for (int sl = 0; sl < SL; ++sl) {
      const long long row = min(r0 + 16 * sl + col, N - 1);
      const gmm_u32x4* src = reinterpret_cast<const gmm_u32x4*>(lib + row * E + 8 * g);
#pragma unroll
      for (int q = 0; q < KS; ++q) a[sl][q] = src[4 * q];
    }
    float mx[SL][4], sm[SL][4], bs[SL][4];
    int bi[SL][4];
#pragma unroll
    for (int sl = 0; sl < SL; ++sl)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        mx[sl][r] = -FLT_MAX;
        sm[sl][r] = 0.f;
        bs[sl][r] = -INFINITY;
        bi[sl][r] = 0x7fffffff;
      }
    const bool again = rt + gridDim.x < rtiles;

    for (int p = 0; p < panels; ++p) {
      gmm_f32x4 lin[SL], sq[SL];
      gmm_panel_logits<KS, SL>(a, par, K, p, p + 1 < panels ? p + 1 : (again ? 0 : -1), stage, buf, tid, lane, lin, sq);
      const int ci = 16 * p + col;
      if (ci < K) {
        const float c = cst[ci];
#pragma unroll
        for (int sl = 0; sl < SL; ++sl)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float v = gmm_logit(lin[sl][r], sq[sl][r], c);
            const float d = v - mx[sl][r];                 // (+inf from the finite start: exp(-inf) = 0, never a NaN)
            const float e = expf(-fabsf(d));
            if (d > 0.f) {
              sm[sl][r] = sm[sl][r] * e + 1.f;
              mx[sl][r] = v;
            } else {
              sm[sl][r] += e;
            }
            if (v > bs[sl][r]) {
              bs[sl][r] = v;
              bi[sl][r] = ci;
            }
          }
      }
    }

    // the 16 lanes of a row: the larger maximum keeps its sum and takes the other's scaled down; the larger logit, the lower component
#pragma unroll
    for (int sl = 0; sl < SL; ++sl)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float m = mx[sl][r], s = sm[sl][r], b = bs[sl][r];
        int i = bi[sl][r];
#pragma unroll
        for (int x = 1; x < 16; x <<= 1) {
          const float mo = __shfl_xor(m, x, 64), so = __shfl_xor(s, x, 64), bo = __shfl_xor(b, x, 64);
          const int io = __shfl_xor(i, x, 64);
          if (m >= mo) {
            s = s + so * expf(mo - m);
          } else {
            s = so + s * expf(m - mo);
            m = mo;
          }
          if (bo > b || (bo == b && io < i)) {
            b = bo;
            i = io;
          }
        }
        const long long row = r0 + 16 * sl + 4 * g + r;
        if (col == 4 * (sl & 3) + r && row < N) {
          const bool out = row_bias && row_bias[row] == -INFINITY;
          lse[row] = out ? -INFINITY : m + logf(s);
          if (assign) assign[row] = out ? -1 : i;
        }
      }
  }
}

template <int KS>
constexpr size_t gmm_mstep_lds() { return (size_t)(512 + 256 + GM_CH * (4 * KS + 1)) * sizeof(gmm_f32x4); }

// part[range][k][0 .. E - 1 | E .. 2E - 1 | 2E] = (s1, s2, w) of the range's rows under component k
template <int KS>
__global__ __launch_bounds__(256, 2) void gmm_mstep_kernel(const bf16_t* __restrict__ lib, long long N, const float* __restrict__ row_bias,
                                                        const float* __restrict__ par, int K, const float* __restrict__ cst,
                                                        const float* __restrict__ lse, float* __restrict__ part, long long ranges,
                                                        long long nchunks) {
  extern __shared__ gmm_f32x4 gm_lds[];
  constexpr int E = 32 * KS, PV = 4 * KS + 1, DB = 2 * KS, NB = (DB + 3) / 4;   // PV: the row tile's pitch in 16-B units
  gmm_f32x4* stage = gm_lds;                                                     // [2][256]
  float* rl = reinterpret_cast<float*>(gm_lds + 512);                            // [4 slabs][4 steps][64 lanes]
  gmm_u32x4* xt = reinterpret_cast<gmm_u32x4*>(gm_lds + 768);                    // [64 rows][PV]
  const unsigned short* xs = reinterpret_cast<const unsigned short*>(xt);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), col = lane & 15, g = lane >> 4;
  const int panels = (K + 15) >> 4;
  const long long items = ranges * panels;

  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const long long range = it / panels;
    const int p = (int)(it - range * panels);
    const long long c0 = range * nchunks / ranges, c1 = (range + 1) * nchunks / ranges;
    gmm_f32x4 acc1[NB], acc2[NB], accw = gmm_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      acc1[i] = gmm_f32x4{0.f, 0.f, 0.f, 0.f};
      acc2[i] = gmm_f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int ci = 16 * p + col;
    const float cc = ci < K ? cst[ci] : 0.f;
    int buf = 0;
    gmm_stash(gmm_fetch<KS>(par, K, p, 0, tid), stage, tid);   // (the last readers of the images: the item before, behind its last barrier)
    __syncthreads();

    for (long long c = c0; c < c1; ++c) {
      const long long r0 = c * GM_CH + 16 * wave;
      gmm_u32x4 a[1][KS];
      {
        const long long row = min(r0 + col, N - 1);
        const gmm_u32x4* src = reinterpret_cast<const gmm_u32x4*>(lib + row * E + 8 * g);
#pragma unroll
        for (int q = 0; q < KS; ++q) {
          a[0][q] = src[4 * q];
          xt[(16 * wave + col) * PV + 4 * q + g] = a[0][q];
        }
      }
      gmm_f32x4 lin[1], sq[1];
      gmm_panel_logits<KS, 1>(a, par, K, p, c + 1 < c1 ? p : -1, stage, buf, tid, lane, lin, sq);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const long long row = r0 + 4 * g + t;
        float r = 0.f;
        if (row < N && ci < K && !(row_bias && row_bias[row] == -INFINITY)) {
          const float l = lse[row];
          if (l > -INFINITY) r = expf(gmm_logit(lin[0][t], sq[0][t], cc) - l);
        }
        rl[(4 * wave + t) * 64 + lane] = r;
      }
      __syncthreads();
#pragma unroll 1
      for (int sb = 0; sb < 4; ++sb)   // (not unrolled: sixteen steps of up to 16 MFMAs each in one block spilled at E = 288 .. 448)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float r = rl[(4 * sb + t) * 64 + lane];
          const unsigned short* xr = xs + (16 * sb + 4 * g + t) * (8 * PV) + col;
#pragma unroll
          for (int i = 0; i < NB; ++i) {
            const int db = wave + 4 * i;
            if (4 * i + 3 < DB || db < DB) {   // (a compile-time yes but for the last block of an odd E / 32)
              const float x = __uint_as_float((unsigned)xr[16 * db] << 16);
              acc1[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(r, x, acc1[i], 0, 0, 0);
              acc2[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(r, x * x, acc2[i], 0, 0, 0);
            }
          }
          if (wave == 3) accw = __builtin_amdgcn_mfma_f32_16x16x4f32(r, 1.f, accw, 0, 0, 0);
        }
      __syncthreads();   // the row tile and r are rewritten by the next chunk
    }

    // result map: column = dimension 16 db + (lane & 15), row = component 16 p + 4 g + register
    float* out = part + range * K * (2 * E + 1);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int k = 16 * p + 4 * g + t;
      if (k < K) {
        float* o = out + (long long)k * (2 * E + 1);
#pragma unroll
        for (int i = 0; i < NB; ++i) {
          const int db = wave + 4 * i;
          if (4 * i + 3 < DB || db < DB) {   // (a compile-time yes but for the last block of an odd E / 32)
            o[16 * db + col] = acc1[i][t];
            o[E + 16 * db + col] = acc2[i][t];
          }
        }
        if (wave == 3 && col == 0) o[2 * E] = accw[t];
      }
    }
  }
}

// w, s1, s2 = the ranges' blocks added in ascending order
__global__ __launch_bounds__(256) void gmm_finish_kernel(const float* __restrict__ part, long long ranges, int K, int E, float* __restrict__ w,
                                                         float* __restrict__ s1, float* __restrict__ s2) {
  const int k = blockIdx.x, W = 2 * E + 1;
  for (int e = threadIdx.x; e < W; e += 256) {
    float s = 0.f;
    for (long long i = 0; i < ranges; ++i) s += part[(i * K + k) * W + e];
    if (e < E) s1[(long long)k * E + e] = s;
    else if (e < 2 * E) s2[(long long)k * E + e - E] = s;
    else w[k] = s;
  }
}

static int gmm_check(const char* what, long long N, int E, int K, int blocks) {
  COATI_CHECK_SHAPE(E >= 32 && E <= GM_E_MAX && E % 32 == 0, "%s: E=%d is not a multiple of 32 in 32 .. %d", what, E, GM_E_MAX);
  COATI_CHECK_SHAPE(N >= 1 && N < (1ll << 31), "%s: N=%lld outside 1 .. 2^31 - 1", what, N);
  COATI_CHECK_SHAPE(K >= 1 && K <= GM_K_MAX, "%s: K=%d outside 1 .. %d", what, K, GM_K_MAX);
  COATI_CHECK_SHAPE(blocks >= 0, "%s: blocks=%d < 0", what, blocks);
  return COATI_OK;
}

static long long gmm_chunks(long long N) { return (N + GM_CH - 1) / GM_CH; }
static long long gmm_ranges(long long N) { return gmm_chunks(N) < GM_RANGES ? gmm_chunks(N) : GM_RANGES; }

template <int KS>
static int gmm_estep_launch(const bf16_t* lib, long long N, const float* row_bias, const float* par, int K, const float* cst, float* lse,
                            int* assign, int blocks, hipStream_t s) {
  const long long rtiles = (N + 64 * GM_SL - 1) / (64 * GM_SL);
  const int grid = (int)(blocks > 0 ? (blocks < rtiles ? blocks : rtiles) : (rtiles < GM_ESTEP_GRID ? rtiles : GM_ESTEP_GRID));
  hipLaunchKernelGGL((gmm_estep_kernel<KS>), dim3(grid), dim3(256), 0, s, lib, N, row_bias, par, K, cst, lse, assign);
  COATI_LAUNCH_CHECK("gmm_estep");
  return COATI_OK;
}

template <int KS>
static int gmm_mstep_launch(const bf16_t* lib, long long N, const float* row_bias, const float* par, int K, const float* cst,
                            const float* lse, float* part, float* w, float* s1, float* s2, int blocks, hipStream_t s) {
  constexpr size_t lds = gmm_mstep_lds<KS>();
  auto kern = gmm_mstep_kernel<KS>;
  if (lds > 64 * 1024) {
    static bool attr_set = false;
    if (!attr_set) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) {
        coati_set_error("gmm_mstep: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
        return COATI_EHIP;
      }
      attr_set = true;
    }
  }
  const long long ranges = gmm_ranges(N), items = ranges * ((K + 15) / 16);
  const int grid = (int)(blocks > 0 && blocks < items ? blocks : items);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, lib, N, row_bias, par, K, cst, lse, part, ranges, gmm_chunks(N));
  COATI_LAUNCH_CHECK("gmm_mstep");
  hipLaunchKernelGGL(gmm_finish_kernel, dim3(K), dim3(256), 0, s, part, ranges, K, 32 * KS, w, s1, s2);
  COATI_LAUNCH_CHECK("gmm_finish");
  return COATI_OK;
}

#define GM_CASES GM_CASE(1) GM_CASE(2) GM_CASE(3) GM_CASE(4) GM_CASE(5) GM_CASE(6) GM_CASE(7) GM_CASE(8) \
                 GM_CASE(9) GM_CASE(10) GM_CASE(11) GM_CASE(12) GM_CASE(13) GM_CASE(14) GM_CASE(15) GM_CASE(16)

int coati_gmm_estep(const uint16_t* lib, int64_t N, int E, const float* row_bias, const float* par, int K, const float* cst, float* lse,
                    int32_t* assign, int blocks, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(lib, "gmm_estep: lib is null");
  COATI_CHECK_ARG(par, "gmm_estep: par is null");
  COATI_CHECK_ARG(cst, "gmm_estep: cst is null");
  COATI_CHECK_ARG(lse, "gmm_estep: lse is null");
  COATI_TRY(gmm_check("gmm_estep", N, E, K, blocks));
  switch (E >> 5) {
#define GM_CASE(KS) \
  case KS: return gmm_estep_launch<KS>(lib, N, row_bias, par, K, cst, lse, assign, blocks, s);
    GM_CASES
#undef GM_CASE
  }
  coati_set_error("gmm_estep: E=%d has no kernel", E);
  return COATI_ESHAPE;
}

int coati_gmm_mstep(const uint16_t* lib, int64_t N, int E, const float* row_bias, const float* par, int K, const float* cst,
                    const float* lse, float* part, int64_t part_floats, float* w, float* s1, float* s2, int blocks, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(lib, "gmm_mstep: lib is null");
  COATI_CHECK_ARG(par, "gmm_mstep: par is null");
  COATI_CHECK_ARG(cst, "gmm_mstep: cst is null");
  COATI_CHECK_ARG(lse, "gmm_mstep: lse is null");
  COATI_CHECK_ARG(part, "gmm_mstep: part is null");
  COATI_CHECK_ARG(w, "gmm_mstep: w is null");
  COATI_CHECK_ARG(s1, "gmm_mstep: s1 is null");
  COATI_CHECK_ARG(s2, "gmm_mstep: s2 is null");
  COATI_TRY(gmm_check("gmm_mstep", N, E, K, blocks));
  const long long need = gmm_ranges(N) * K * (2ll * E + 1);
  COATI_CHECK_SHAPE(part_floats >= need, "gmm_mstep: part_floats=%lld < ranges K (2 E + 1) = %lld", (long long)part_floats, need);
  switch (E >> 5) {
#define GM_CASE(KS) \
  case KS: return gmm_mstep_launch<KS>(lib, N, row_bias, par, K, cst, lse, part, w, s1, s2, blocks, s);
    GM_CASES
#undef GM_CASE
  }
  coati_set_error("gmm_mstep: E=%d has no kernel", E);
  return COATI_ESHAPE;
}

int coati_gmm_chunk(void) { return GM_CH; }

int64_t coati_gmm_ranges(int64_t N) {
  if (!(N >= 1 && N < (1ll << 31))) {
    coati_set_error("gmm_ranges: N=%lld outside 1 .. 2^31 - 1", (long long)N);
    return COATI_ESHAPE;
  }
  return gmm_ranges(N);
}

int64_t coati_gmm_part_floats(int64_t N, int E, int K) {
  if (!(N >= 1 && N < (1ll << 31) && E >= 32 && E <= GM_E_MAX && E % 32 == 0 && K >= 1 && K <= GM_K_MAX)) {
    coati_set_error("gmm_part_floats: N=%lld E=%d K=%d out of range", (long long)N, E, K);
    return COATI_ESHAPE;
  }
  return gmm_ranges(N) * K * (2ll * E + 1);
}
