// Property heads on rows of embeddings (include/coati_screen.h): out = last(resnet(first(x))) for every row of a bf16 library, as one
// kernel.  The library is read once, nothing but [N, P] floats is written, and no activation ever exists in memory.
//
// head_eval_kernel<F, WAVES, NP>, one workgroup per tile of WAVES * NP * 32 rows; a wave owns NP panels of 32 rows for the whole kernel:
//  * every product is computed TRANSPOSED on v_mfma_f32_32x32x16_bf16: the weights are the M side (32 output features x 16 inputs, read
//    from LDS), the rows of the library the N side.  The result map (column = lane & 31 = the lane's ROW of the library, register r =
//    feature 8 (r >> 2) + 4 (lane >> 5) + (r & 3) of the 32-feature tile) then is, register for register, the B operand of the next
//    product: registers 8 t .. 8 t + 7 of tile mt, rounded to bf16, are the lane's eight k values of k-step 2 mt + t -- in the order
//    k = 8 (j >> 2) + 4 (lane >> 5) + (j & 3) instead of 8 (lane >> 5) + j.  A product does not care in which order k is summed as long
//    as both operands agree, so the residual weights are staged with the two middle 4-element groups of every 16 swapped and are then
//    read like any A operand (one ds_read_b128).  Nothing passes through LDS or the lanes between two layers;
//  * the f32 residual stream h [F, rows] lives in registers (F / 32 * NP * 16 per lane), the bf16 operand of the layer in F / 16 * NP * 4
//    more, a 32-feature tile's accumulators in NP * 16;
//  * weights come through LDS in chunks of at most 32 KiB, two buffers, one barrier per chunk: the first layer by K (all F features x 64
//    inputs: the x fragments of a chunk are loaded from memory just in time, the accumulators are the stream itself), a residual layer
//    by M (16384 / F output features x all F inputs).  The next chunk travels global -> registers under the current chunk's MFMAs and
//    registers -> LDS behind them.  Row strides of K + 8 elements keep every ds_read_b128 group on 16 different 16-byte slots;
//  * the chunk count is the same for every thread (ceil(E / 64) + D * F / MC), so no barrier is under a lane- or wave-dependent condition;
//  * the last layer (P <= 8 outputs) is VALU work: a lane's dot over the features it holds, plus the other half-wave's;
//  * rows >= N (ragged last tile) are read at row N - 1 and never written.
// No atomics, no workspace.
#include "kernels.h"

#define HEAD_E_MAX 512
#define HEAD_D_MAX 16
#define HEAD_P_MAX 8
#define HEAD_KC 64         // inputs per chunk of the first layer (the last chunk has 32 when E % 64 == 32)
#define HEAD_CHUNK 16384   // elements per chunk of a residual layer
#ifndef HEAD_WAVES_256
#define HEAD_WAVES_256 4   // F = 256: 4 waves (one per SIMD) of one 32-row panel each; wider tiles spill
#define HEAD_NP_256 1
#endif

template <int F, int WAVES, int NP>
__global__ __launch_bounds__(64 * WAVES) void head_eval_kernel(const bf16_t* __restrict__ x, long long ldx, long long N, int E,
                                                               const bf16_t* __restrict__ w0, const float* __restrict__ b0,
                                                               const bf16_t* __restrict__ wr, const float* __restrict__ br, int D,
                                                               const float* __restrict__ wl, const float* __restrict__ bl, int P,
                                                               float* __restrict__ out, long long ldo) {
  constexpr int NT = 64 * WAVES, MT = F / 32, KS = F / 16;
  constexpr int MC = HEAD_CHUNK / F < F ? HEAD_CHUNK / F : F;   // output features per residual chunk: 64 (F = 256), 128, 64
  constexpr int MCH = F / MC, TPC = MC / 32;                    // chunks per residual layer, 32-feature tiles per chunk
  constexpr int LD0 = HEAD_KC + 8, LDR = F + 8;                 // LDS row strides (elements)
  constexpr int BUF = F * LD0 > MC * LDR ? F * LD0 : MC * LDR;
  constexpr int U0 = F * HEAD_KC / 16, UR = MC * F / 16;        // 32-byte units of a chunk
  constexpr int UPT = ((U0 > UR ? U0 : UR) + NT - 1) / NT;
  __shared__ __attribute__((aligned(16))) bf16_t lds[2][BUF];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, hh = lane >> 5;
  const int C0 = (E + HEAD_KC - 1) / HEAD_KC, CT = C0 + D * MCH;
  const long long row0 = (long long)blockIdx.x * (WAVES * NP * 32) + wave * (NP * 32);

  // chunk gc of the sequence: global -> st (stage_load), st -> lds[gc & 1] (stage_store)
  uint4 st[UPT][2];
  auto stage_load = [&](int gc, bool first) {
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
      const int u = tid + NT * i;
      const bf16_t* src;
      bool on;
      if (first) {   // (a 16-column unit past E, in the last chunk of E % 64 == 32, is neither loaded nor read)
        on = u < U0 && HEAD_KC * gc + 16 * (u & 3) < E;
        src = w0 + (long long)(u >> 2) * E + HEAD_KC * gc + 16 * (u & 3);
      } else {
        const int cc = gc - C0;
        on = u < UR;
        src = wr + ((long long)(cc / MCH) * F + (cc % MCH) * MC + u / KS) * F + 16 * (u % KS);
      }
      if (on) {
        st[i][0] = reinterpret_cast<const uint4*>(src)[0];
        st[i][1] = reinterpret_cast<const uint4*>(src)[1];
      }
    }
  };
  auto stage_store = [&](int gc, bool first) {
    bf16_t* buf = lds[gc & 1];
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
      const int u = tid + NT * i;
      const uint4 a = st[i][0], b = st[i][1];
      if (first) {
        if (u < U0 && HEAD_KC * gc + 16 * (u & 3) < E) {
          uint4* d = reinterpret_cast<uint4*>(buf + (u >> 2) * LD0 + 16 * (u & 3));
          d[0] = a;
          d[1] = b;
        }
      } else if (u < UR) {   // groups of 4 elements (g0 g1 | g2 g3) -> (g0 g2 | g1 g3): the k order of the chained operand
        uint4* d = reinterpret_cast<uint4*>(buf + (u / KS) * LDR + 16 * (u % KS));
        d[0] = make_uint4(a.x, a.y, b.x, b.y);
        d[1] = make_uint4(a.z, a.w, b.z, b.w);
      }
    }
  };

  // the lane's library rows: B[k = 16 s + 8 hh + j][column = n] of panel p
  const bf16_t* xrow[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const long long row = min(row0 + 32 * p + n, N - 1);
    xrow[p] = x + row * ldx + 8 * hh;
  }
  uint4 xn[NP][4];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int t = 0; t < 4; ++t) xn[p][t] = make_uint4(0u, 0u, 0u, 0u);
  auto x_load = [&](int c) {
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (HEAD_KC * c + 16 * t < E) xn[p][t] = *reinterpret_cast<const uint4*>(xrow[p] + HEAD_KC * c + 16 * t);
  };

  stage_load(0, true);
  x_load(0);
  stage_store(0, true);

  // the stream: h[mt][p][r] = feature 32 mt + 8 (r >> 2) + 4 hh + (r & 3) of row 32 p + n
  f32x16 h[MT][NP];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 bv = *reinterpret_cast<const float4*>(b0 + 32 * mt + 8 * q + 4 * hh);
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        h[mt][p][4 * q] = bv.x;
        h[mt][p][4 * q + 1] = bv.y;
        h[mt][p][4 * q + 2] = bv.z;
        h[mt][p][4 * q + 3] = bv.w;
      }
    }
  __syncthreads();

  int gc = 0;
  // first layer, by K
  for (int c = 0; c < C0; ++c, ++gc) {
    uint4 xc[NP][4];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int t = 0; t < 4; ++t) xc[p][t] = xn[p][t];
    const bool whole = HEAD_KC * c + 32 < E;   // 64 inputs in this chunk, not 32
    if (c + 1 < C0) {
      stage_load(gc + 1, true);
      x_load(c + 1);
    } else if (gc + 1 < CT) {
      stage_load(gc + 1, false);
    }
    const bf16_t* a = lds[gc & 1] + n * LD0 + 8 * hh;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (t < 2 || whole) {
          const bf16x8 af = *reinterpret_cast<const bf16x8*>(a + 32 * mt * LD0 + 16 * t);
#pragma unroll
          for (int p = 0; p < NP; ++p)
            h[mt][p] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, __builtin_bit_cast(bf16x8, xc[p][t]), h[mt][p], 0, 0, 0);
        }
      }
    if (c + 1 < C0)
      stage_store(gc + 1, true);
    else if (gc + 1 < CT)
      stage_store(gc + 1, false);
    __syncthreads();
  }

  // residual layers, by M
  for (int l = 0; l < D; ++l) {
    bf16x8 bfr[NP][KS];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          uint4 v;
          v.x = pack2bf(h[mt][p][8 * t], h[mt][p][8 * t + 1]);
          v.y = pack2bf(h[mt][p][8 * t + 2], h[mt][p][8 * t + 3]);
          v.z = pack2bf(h[mt][p][8 * t + 4], h[mt][p][8 * t + 5]);
          v.w = pack2bf(h[mt][p][8 * t + 6], h[mt][p][8 * t + 7]);
          bfr[p][2 * mt + t] = __builtin_bit_cast(bf16x8, v);
        }
    const float* bb = br + (long long)l * F + 4 * hh;
#pragma unroll
    for (int i = 0; i < MCH; ++i, ++gc) {
      if (gc + 1 < CT) stage_load(gc + 1, false);
      const bf16_t* a = lds[gc & 1] + n * LDR + 8 * hh;
#pragma unroll
      for (int tt = 0; tt < TPC; ++tt) {
        const int mt = i * TPC + tt;
        f32x16 acc[NP];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 bv = *reinterpret_cast<const float4*>(bb + 32 * mt + 8 * q);
#pragma unroll
          for (int p = 0; p < NP; ++p) {
            acc[p][4 * q] = bv.x;
            acc[p][4 * q + 1] = bv.y;
            acc[p][4 * q + 2] = bv.z;
            acc[p][4 * q + 3] = bv.w;
          }
        }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const bf16x8 af = *reinterpret_cast<const bf16x8*>(a + 32 * tt * LDR + 16 * s);
#pragma unroll
          for (int p = 0; p < NP; ++p) acc[p] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr[p][s], acc[p], 0, 0, 0);
        }
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
          for (int r = 0; r < 16; ++r) h[mt][p][r] += fmaxf(acc[p][r], 0.f);
      }
      if (gc + 1 < CT) stage_store(gc + 1, false);
      __syncthreads();
    }
  }

  // last layer: the lane's features of its rows against wl, then the other half-wave's
  for (int o = 0; o < P; ++o) {
    float sum[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) sum[p] = 0.f;
    const float* wo = wl + (long long)o * F + 4 * hh;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 wv = *reinterpret_cast<const float4*>(wo + 32 * mt + 8 * q);
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          sum[p] = fmaf(wv.x, h[mt][p][4 * q], sum[p]);
          sum[p] = fmaf(wv.y, h[mt][p][4 * q + 1], sum[p]);
          sum[p] = fmaf(wv.z, h[mt][p][4 * q + 2], sum[p]);
          sum[p] = fmaf(wv.w, h[mt][p][4 * q + 3], sum[p]);
        }
      }
    const float bo = bl[o];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const float tot = half_xchg_sum(sum[p]) + bo;
      const long long row = row0 + 32 * p + n;
      if (hh == 0 && row < N) out[row * ldo + o] = tot;
    }
  }
}

template <int F, int WAVES, int NP>
static void head_launch(const bf16_t* x, long long ldx, long long N, int E, const bf16_t* w0, const float* b0, const bf16_t* wr,
                        const float* br, int D, const float* wl, const float* bl, int P, float* out, long long ldo, hipStream_t s) {
  hipLaunchKernelGGL((head_eval_kernel<F, WAVES, NP>), dim3(cdiv(N, WAVES * NP * 32)), dim3(64 * WAVES), 0, s, x, ldx, N, E, w0, b0, wr, br, D,
                     wl, bl, P, out, ldo);
}

static bool head_aligned16(const void* p) { return (reinterpret_cast<unsigned long long>(p) & 15ull) == 0; }

int launch_head_eval(const bf16_t* x, long long ldx, long long N, int E, const bf16_t* w0, const float* b0, const bf16_t* wr, const float* br,
                     int D, const float* wl, const float* bl, int P, int F, float* out, long long ldo, hipStream_t s) {
  COATI_CHECK_ARG(x && w0 && b0 && wl && bl && out, "head_eval: null operand");
  COATI_CHECK_SHAPE(D >= 0 && D <= HEAD_D_MAX, "head_eval: D=%d outside 0 .. %d", D, HEAD_D_MAX);
  COATI_CHECK_ARG(D == 0 || (wr && br), "head_eval: null residual weights with D=%d", D);
  COATI_CHECK_SHAPE(E >= 32 && E <= HEAD_E_MAX && E % 32 == 0, "head_eval: E=%d is not a multiple of 32 in 32 .. %d", E, HEAD_E_MAX);
  COATI_CHECK_SHAPE(F == 64 || F == 128 || F == 256, "head_eval: F=%d is not 64, 128 or 256", F);
  COATI_CHECK_SHAPE(P >= 1 && P <= HEAD_P_MAX, "head_eval: P=%d outside 1 .. %d", P, HEAD_P_MAX);
  COATI_CHECK_SHAPE(N >= 1 && N < (1ll << 31), "head_eval: N=%lld outside 1 .. 2^31 - 1", N);
  COATI_CHECK_SHAPE(ldx >= E && ldx % 8 == 0, "head_eval: ldx=%lld must be a multiple of 8 and >= E=%d", ldx, E);
  COATI_CHECK_SHAPE(ldo >= P, "head_eval: ldo=%lld < P=%d", ldo, P);
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
