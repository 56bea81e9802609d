// The property head's device body, shared by head_eval_kernel (screen.hip), head_grad_kernel (guide.hip), head_gp_kernel (gp.hip) and
// head_gp_grad_kernel (gp_grad.hip): one text, four kernels.
//
// head_body<F, WAVES, NP, MODE>, one workgroup per tile of WAVES * NP * 32 rows; a wave owns NP panels of 32 rows for the whole kernel:
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
//  * the chunk count is the same for every thread, so no barrier is under a lane- or wave-dependent condition;
//  * the last layer (P <= 8 outputs) is VALU work: a lane's dot over the features it holds, plus the other half-wave's;
//  * rows >= N (ragged last tile) are read at row N - 1 and never written.
//
// MODE = HEAD_MODE_GRAD goes on where the forward ends (include/coati_guide.h).  The forward leaves, next to `h += max(acc, 0)`, the tile's 16 sign
// decisions as one 16-bit word per (layer, 32-feature tile, panel, thread) in LDS: the thread that writes a word is the one that reads it,
// so the words need no barrier of their own.  After `out`, h is dead and d = cot . wl (VALU, like the last layer) takes its registers.  A
// backward layer is the residual-layer loop once more: chunks of wrt[l] (wr[l] transposed, the same middle-group swap), the operand rb(m (.)
// d) built from d and the layer's mask words, accumulators starting at zero, d += acc.  g = rb(d) . w0 runs as one more such layer over w0t
// with E output features: its 32-feature tiles go straight to memory (a lane's registers 4 q .. 4 q + 3 are 4 consecutive floats of its row:
// one 16-byte store).  The chunk sequence is C0 + 2 D MCH + ceil(E / MC), again the same for every thread.
// No atomics, no workspace.
//
// MODE = HEAD_MODE_GP adds the GP head (include/coati_gp.h) where the forward ends.  The inducing points z [Mp, F] are one more residual
// "layer" of Mp <= 64 <= MC output features: one more chunk of the sequence (C0 + D MCH + 1), staged with the same middle-group swap, rows
// past Mp not loaded; its operand is phi = rb(h), its accumulators phi . z_j of the lane's row.  After the exponential, register r of tile
// tt holds k_j, j = 32 tt + 8 (r >> 2) + 4 hh + (r & 3): register for register the B operand (k index = hh) of a v_mfma_f32_32x32x2_f32
// step against q[m][j0 + 4 hh] read from LDS, so w = q k comes out in k's own map without lane movement and without leaving f32.  mean and
// k . w are per-lane dots plus half_xchg_sum, like the last layer.  One more barrier (q in LDS), the same for every thread.
//
// MODE = HEAD_MODE_GPGRAD joins the two (include/coati_acq.h): the forward with mask words, the GP tail, an acquisition a(mean, var) of the
// row, and the gradient of a with respect to the row.  The tail keeps w = qs k (qs the symmetric part of q, so dvar / dk = -2 w) next to
// k; t_j = rs (A ca_j - 2 B w_j) k_j (ca = wm . alpha; A, B: the row's da / d(wm . mean) and da / dvar) takes k's registers and is, rounded
// to bf16, the B operand of one more chained product: against zt [F, Mp] (z transposed), staged like a first-layer chunk (F rows x Mp <=
// 64 columns at row stride 72) with the middle-group swap.  dphi = 2 inv2l2 (tb . zt - phi S), S the row's sum of tb (per-lane sum plus
// half_xchg_sum), phi unpacked from the operand registers of the z product, lands in the registers of h and seeds the backward loop of
// HEAD_MODE_GRAD.  qs has a region of its own in the dynamic LDS (between the weight buffers and the mask words): the buffer q uses in
// HEAD_MODE_GP is the prefetch target of the zt chunk here.  The chunk sequence is C0 + D MCH + 1 + 1 + D MCH + ceil(E / MC).
#pragma once
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

// elements of one of the two weight buffers
template <int F>
constexpr int head_buf_elems() {
  constexpr int MC = HEAD_CHUNK / F < F ? HEAD_CHUNK / F : F;
  return F * (HEAD_KC + 8) > MC * (F + 8) ? F * (HEAD_KC + 8) : MC * (F + 8);
}
// bytes of dynamic LDS of the GRAD body: the two weight buffers, then D layers of mask words
template <int F, int WAVES, int NP>
constexpr size_t head_grad_lds_bytes(int D) {
  return (size_t)4 * head_buf_elems<F>() + (size_t)D * (F / 32) * NP * (64 * WAVES) * 2;
}

// what follows the forward: nothing, the input gradient, or the GP head
#define HEAD_MODE_EVAL 0
#define HEAD_MODE_GRAD 1
#define HEAD_MODE_GP 2
#define HEAD_MODE_GPGRAD 3
#define HEAD_GP_M_MAX 64   // inducing points (padded to 32 or 64)
#define HEAD_GP_LDQ 68     // LDS row stride of q (floats): 32 rows' ds_read_b128 start on 8 different 16-byte slots

typedef float head_f32x4 __attribute__((ext_vector_type(4)));

// bytes of dynamic LDS of the GPGRAD body: the two weight buffers, qs, then D layers of mask words
#define HEAD_GP_Q_BYTES (4 * HEAD_GP_M_MAX * HEAD_GP_LDQ)
template <int F, int WAVES, int NP>
constexpr size_t head_gpgrad_lds_bytes(int D) {
  return head_grad_lds_bytes<F, WAVES, NP>(D) + HEAD_GP_Q_BYTES;
}

// the operands of the GP tail (HEAD_MODE_GP); the other modes pass an empty one
struct HeadGpOps {
  const bf16_t* z;      // [Mp, F]
  const float* zn;      // [Mp]
  const float* alpha;   // [P, Mp]
  const float* q;       // [Mp, Mp]
  const float* c;       // [P]
  float inv2l2, s2;
  int P, Mp;
  float* mean;          // [N, P], row stride ldm
  long long ldm;
  float* var;           // [N]
};

// what HEAD_MODE_GPGRAD needs on top of HeadGpOps (whose q then is qs, the symmetric part); the other modes pass an empty one
struct HeadAcqOps {
  const bf16_t* zt;     // [F, Mp]: z transposed
  const float* wm;      // [P] weights on the means
  float kappa, var_add, best;
  int mode;             // 0: wm . mean + kappa sqrt(var + var_add);  1: expected improvement over best
  const float* rs;      // [N] row scales of the gradient, or null
  float* acq;           // [N]
};

template <int F, int WAVES, int NP, int MODE>
__device__ __forceinline__ void head_body(const bf16_t* __restrict__ x, long long ldx, long long N, int E, const bf16_t* __restrict__ w0,
                                          const float* __restrict__ b0, const bf16_t* __restrict__ wr, const float* __restrict__ br, int D,
                                          const float* __restrict__ wl, const float* __restrict__ bl, int P, float* __restrict__ out,
                                          long long ldo, const bf16_t* __restrict__ w0t, const bf16_t* __restrict__ wrt,
                                          const float* __restrict__ cot, long long ldc, float* __restrict__ g, long long ldg,
                                          const HeadGpOps& gp, const HeadAcqOps& aq = HeadAcqOps{}) {
  constexpr bool GRAD = MODE == HEAD_MODE_GRAD, GP = MODE == HEAD_MODE_GP, GPG = MODE == HEAD_MODE_GPGRAD;
  constexpr bool BACK = GRAD || GPG;   // mask words in the forward, dynamic LDS, the backward loop
  constexpr int ZC = GPG ? 2 : 0;      // the z and zt chunks between the forward's and the backward's
  constexpr int NT = 64 * WAVES, MT = F / 32, KS = F / 16;
  constexpr int MC = HEAD_CHUNK / F < F ? HEAD_CHUNK / F : F;   // output features per residual chunk: 64 (F = 256), 128, 64
  constexpr int MCH = F / MC, TPC = MC / 32;                    // chunks per residual layer, 32-feature tiles per chunk
  constexpr int LD0 = HEAD_KC + 8, LDR = F + 8;                 // LDS row strides (elements)
  constexpr int BUF = head_buf_elems<F>();
  constexpr int U0 = F * HEAD_KC / 16, UR = MC * F / 16;        // 32-byte units of a chunk
  constexpr int UPT = ((U0 > UR ? U0 : UR) + NT - 1) / NT;
  bf16_t* lds;                                                  // [2][BUF]
  unsigned short* masks = nullptr;                              // GRAD, GPGRAD: [D][MT][NP][NT]
  float* qown = nullptr;                                        // GPGRAD: qs [HEAD_GP_M_MAX][HEAD_GP_LDQ]
  if constexpr (BACK) {
    extern __shared__ __attribute__((aligned(16))) unsigned char head_smem[];
    lds = reinterpret_cast<bf16_t*>(head_smem);
    if constexpr (GPG) qown = reinterpret_cast<float*>(head_smem + 4 * BUF);
    masks = reinterpret_cast<unsigned short*>(head_smem + 4 * BUF + (GPG ? HEAD_GP_Q_BYTES : 0));
  } else {
    __shared__ __attribute__((aligned(16))) bf16_t head_lds[2 * BUF];
    lds = head_lds;
  }

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, hh = lane >> 5;
  const int C0 = (E + HEAD_KC - 1) / HEAD_KC;
  const int CT = BACK ? C0 + 2 * D * MCH + ZC + (E + MC - 1) / MC : C0 + D * MCH + (GP ? 1 : 0);
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
      } else if (MODE == HEAD_MODE_EVAL || gc - C0 < D * MCH) {
        const int cc = gc - C0;
        on = u < UR;
        src = wr + ((long long)(cc / MCH) * F + (cc % MCH) * MC + u / KS) * F + 16 * (u % KS);
      } else if (GP || (GPG && gc - C0 == D * MCH)) {   // z [Mp, F], one chunk (Mp <= 64 <= MC): its rows, none past Mp
        on = u < UR && u / KS < gp.Mp;
        src = gp.z + (long long)(u / KS) * F + 16 * (u % KS);
      } else if (gc - C0 - ZC < 2 * D * MCH) {   // backward layer D - 1 - cc / MCH: the same chunks of the transposed weights
        const int cc = gc - C0 - D * MCH - ZC;
        on = u < UR;
        src = wrt + ((long long)(D - 1 - cc / MCH) * F + (cc % MCH) * MC + u / KS) * F + 16 * (u % KS);
      } else {                              // w0t [E, F]: MC of its rows, none past E
        const int cc = gc - C0 - 2 * D * MCH - ZC;
        on = u < UR && cc * MC + u / KS < E;
        src = w0t + ((long long)cc * MC + u / KS) * F + 16 * (u % KS);
      }
      if (on) {
        st[i][0] = reinterpret_cast<const uint4*>(src)[0];
        st[i][1] = reinterpret_cast<const uint4*>(src)[1];
      }
    }
  };
  auto stage_store = [&](int gc, bool first) {
    bf16_t* buf = lds + (gc & 1) * BUF;
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
        uint4* d = reinterpret_cast<uint4*>(buf + (u / KS) * LDR + 16 * (u % KS));   // (rows of w0t past E: stale registers, never read)
        d[0] = make_uint4(a.x, a.y, b.x, b.y);
        d[1] = make_uint4(a.z, a.w, b.z, b.w);
      }
    }
  };

  // GPGRAD: the zt chunk [F, Mp]: a first-layer chunk's layout (F rows, 16-column units, none past Mp), a residual chunk's group swap
  auto stage_load_zt = [&]() {
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
      const int u = tid + NT * i;
      if (u < U0 && 16 * (u & 3) < gp.Mp) {
        const bf16_t* src = aq.zt + (long long)(u >> 2) * gp.Mp + 16 * (u & 3);
        st[i][0] = reinterpret_cast<const uint4*>(src)[0];
        st[i][1] = reinterpret_cast<const uint4*>(src)[1];
      }
    }
  };
  auto stage_store_zt = [&](int gc) {
    bf16_t* buf = lds + (gc & 1) * BUF;
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
      const int u = tid + NT * i;
      const uint4 a = st[i][0], b = st[i][1];
      if (u < U0 && 16 * (u & 3) < gp.Mp) {
        uint4* d = reinterpret_cast<uint4*>(buf + (u >> 2) * LD0 + 16 * (u & 3));
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
    const bf16_t* a = lds + (gc & 1) * BUF + n * LD0 + 8 * hh;
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
      const bf16_t* a = lds + (gc & 1) * BUF + n * LDR + 8 * hh;
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
        for (int p = 0; p < NP; ++p) {
#pragma unroll
          for (int r = 0; r < 16; ++r) h[mt][p][r] += fmaxf(acc[p][r], 0.f);
          if constexpr (BACK) {   // the tile's ReLU decisions, bit r = register r
            unsigned m = 0;
#pragma unroll
            for (int r = 0; r < 16; ++r) m |= (acc[p][r] > 0.f ? 1u : 0u) << r;
            masks[(((long long)l * MT + mt) * NP + p) * NT + tid] = (unsigned short)m;
          }
        }
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

  if constexpr (GP || GPG) {
    // phi = rb(h) is the operand of one more chained product, against z: its chunk (number gc) came in under the last residual chunk.
    // |phi|^2 is summed over the rounded values the lane holds, then over the two half-waves
    const int Mp = gp.Mp;
    bf16x8 bfr[NP][KS];
    float pn[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      pn[p] = 0.f;
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
          float f[8];
          unpack8(v, f);
#pragma unroll
          for (int e = 0; e < 8; ++e) pn[p] = fmaf(f[e], f[e], pn[p]);
        }
      pn[p] = half_xchg_sum(pn[p]);
    }

    // q [Mp, Mp] f32 travels global -> registers under the z product and registers -> LDS behind it: into the weight buffer that the
    // chunk sequence has left (its last reader is behind the previous barrier), or, where that is too small (F = 64), an array of its own
    constexpr int QPT = HEAD_GP_M_MAX * HEAD_GP_M_MAX / 4 / NT;
    constexpr bool QOWN = 2 * BUF < 4 * HEAD_GP_M_MAX * HEAD_GP_LDQ;
    float* qs;
    if constexpr (GPG) {   // (that buffer is where the zt chunk goes: qs has a region of the dynamic LDS)
      qs = qown;
      stage_load_zt();
    } else if constexpr (QOWN) {
      __shared__ __attribute__((aligned(16))) float head_q[HEAD_GP_M_MAX * HEAD_GP_LDQ];
      qs = head_q;
    } else {
      qs = reinterpret_cast<float*>(lds + ((gc + 1) & 1) * BUF);
    }
    const int QU = Mp * Mp / 4;   // 16-byte units of q
    head_f32x4 qv[QPT];
#pragma unroll
    for (int i = 0; i < QPT; ++i) {
      const int u = tid + NT * i;
      qv[i] = u < QU ? *reinterpret_cast<const head_f32x4*>(gp.q + 4 * u) : head_f32x4{0.f, 0.f, 0.f, 0.f};
    }

    // k[tt][p][r] = s2 exp(-d2 inv2l2) of inducing point 32 tt + 8 (r >> 2) + 4 hh + (r & 3) and the lane's row; exp as exp2 (v_exp_f32)
    const float nl = -gp.inv2l2 * 1.44269504088896341f;
    f32x16 kk[HEAD_GP_M_MAX / 32][NP];
    {
      const bf16_t* a = lds + (gc & 1) * BUF + n * LDR + 8 * hh;
#pragma unroll
      for (int tt = 0; tt < HEAD_GP_M_MAX / 32; ++tt) {
        if (32 * tt < Mp) {   // (the same for every thread)
          f32x16 acc[NP];
#pragma unroll
          for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[p][r] = 0.f;
#pragma unroll
          for (int s = 0; s < KS; ++s) {
            const bf16x8 af = *reinterpret_cast<const bf16x8*>(a + 32 * tt * LDR + 16 * s);
#pragma unroll
            for (int p = 0; p < NP; ++p) acc[p] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr[p][s], acc[p], 0, 0, 0);
          }
#pragma unroll
          for (int q4 = 0; q4 < 4; ++q4) {
            const float4 zv = *reinterpret_cast<const float4*>(gp.zn + 32 * tt + 8 * q4 + 4 * hh);
            const float ze[4] = {zv.x, zv.y, zv.z, zv.w};
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float d2 = fmaxf(fmaf(-2.f, acc[p][4 * q4 + e], pn[p] + ze[e]), 0.f);
                kk[tt][p][4 * q4 + e] = gp.s2 * __builtin_amdgcn_exp2f(d2 * nl);
              }
          }
        } else {
#pragma unroll
          for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int r = 0; r < 16; ++r) kk[tt][p][r] = 0.f;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < QPT; ++i) {
      const int u = tid + NT * i;
      if (u < QU) *reinterpret_cast<head_f32x4*>(qs + ((4 * u) / Mp) * HEAD_GP_LDQ + (4 * u) % Mp) = qv[i];
    }
    if constexpr (GPG) stage_store_zt(gc + 1);

    // mean: the lane's k against alpha, then the other half-wave's (like the last layer)
    float am[NP];   // GPGRAD: wm . mean of the row
#pragma unroll
    for (int p = 0; p < NP; ++p) am[p] = 0.f;
    for (int o = 0; o < gp.P; ++o) {
      float sum[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p) sum[p] = 0.f;
      const float* ao = gp.alpha + (long long)o * Mp + 4 * hh;
#pragma unroll
      for (int tt = 0; tt < HEAD_GP_M_MAX / 32; ++tt)
        if (32 * tt < Mp) {
#pragma unroll
          for (int q4 = 0; q4 < 4; ++q4) {
            const float4 av = *reinterpret_cast<const float4*>(ao + 32 * tt + 8 * q4);
#pragma unroll
            for (int p = 0; p < NP; ++p) {
              sum[p] = fmaf(av.x, kk[tt][p][4 * q4], sum[p]);
              sum[p] = fmaf(av.y, kk[tt][p][4 * q4 + 1], sum[p]);
              sum[p] = fmaf(av.z, kk[tt][p][4 * q4 + 2], sum[p]);
              sum[p] = fmaf(av.w, kk[tt][p][4 * q4 + 3], sum[p]);
            }
          }
        }
      const float co = gp.c[o];
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const float tot = half_xchg_sum(sum[p]) + co;
        const long long row = row0 + 32 * p + n;
        if (hh == 0 && row < N) gp.mean[row * gp.ldm + o] = tot;
        if constexpr (GPG) am[p] = fmaf(aq.wm[o], tot, am[p]);
      }
    }
    __syncthreads();   // q is in LDS (GPGRAD: and the zt chunk)
    if constexpr (GPG) {   // the zt chunk is the current one; the backward's first chunk travels under the rest of the tail
      ++gc;
      stage_load(gc + 1, false);
    }

    // w = q k on v_mfma_f32_32x32x2_f32, all f32: register r of k's tile tt is the B operand (k index = hh) of the step against
    // q[32 mi + n][32 tt + 8 (r >> 2) + 4 hh + (r & 3)], and w comes out in k's own map; var = s2 - k . w
    const float* qa = qs + n * HEAD_GP_LDQ + 4 * hh;
    float quad[NP];
    f32x16 wk[GPG ? HEAD_GP_M_MAX / 32 : 1][NP];   // GPGRAD keeps w, in k's map
#pragma unroll
    for (int p = 0; p < NP; ++p) quad[p] = 0.f;
#pragma unroll
    for (int mi = 0; mi < HEAD_GP_M_MAX / 32; ++mi)
      if (32 * mi < Mp) {
        f32x16 w[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
          for (int r = 0; r < 16; ++r) w[p][r] = 0.f;
#pragma unroll
        for (int tt = 0; tt < HEAD_GP_M_MAX / 32; ++tt)
          if (32 * tt < Mp) {
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
              const float4 av = *reinterpret_cast<const float4*>(qa + 32 * mi * HEAD_GP_LDQ + 32 * tt + 8 * q4);
#pragma unroll
              for (int p = 0; p < NP; ++p) {
                w[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, kk[tt][p][4 * q4], w[p], 0, 0, 0);
                w[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, kk[tt][p][4 * q4 + 1], w[p], 0, 0, 0);
                w[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, kk[tt][p][4 * q4 + 2], w[p], 0, 0, 0);
                w[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, kk[tt][p][4 * q4 + 3], w[p], 0, 0, 0);
              }
            }
          }
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
          for (int r = 0; r < 16; ++r) quad[p] = fmaf(kk[mi][p][r], w[p][r], quad[p]);
        if constexpr (GPG) {
#pragma unroll
          for (int p = 0; p < NP; ++p) wk[mi][p] = w[p];
        }
      }
    float cA[NP], cB[NP];   // GPGRAD: rs A and -2 rs B of the row
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const float v = fmaxf(gp.s2 - half_xchg_sum(quad[p]), 0.f);
      const long long row = row0 + 32 * p + n;
      if (hh == 0 && row < N) gp.var[row] = v;
      if constexpr (GPG) {
        // the acquisition a and its derivatives A = da / d(wm . mean), B = da / dvar.  B = 0 where var was clamped or has no digits left
        const float va = v + aq.var_add, sd = sqrtf(va);
        const bool dead = !(v > 0.f) || !(va > 1e-6f * gp.s2);
        const float hb = dead ? 0.f : aq.kappa / (2.f * sd);
        float a, A, B;
        if (aq.mode == 0) {
          a = fmaf(aq.kappa, sd, am[p]);
          A = 1.f;
          B = hb;
        } else {
          const float mu = am[p] - aq.best, s = aq.kappa * sd;
          if (s > 0.f) {
            const float u = mu / s;
            const float Phi = 0.5f * (1.f + erff(u * 0.70710678118654752f));
            const float ph = 0.39894228040143268f * expf(-0.5f * u * u);
            a = fmaf(mu, Phi, s * ph);
            A = Phi;
            B = ph * hb;
          } else {
            a = fmaxf(mu, 0.f);
            A = mu > 0.f ? 1.f : 0.f;
            B = 0.f;
          }
        }
        if (hh == 0 && row < N) aq.acq[row] = a;
        const float r = aq.rs ? aq.rs[min(row, N - 1)] : 1.f;
        cA[p] = r * A;
        cB[p] = -2.f * r * B;
      }
    }

    if constexpr (GPG) {
      // t_j = (cA ca_j + cB w_j) k_j in k's registers, ca = wm . alpha; tb = rb(t) is the B operand of the zt product (k-step 2 tt + t =
      // registers 8 t .. 8 t + 7 of tile tt, like any chained operand); S = sum_j tb_j over the rounded values
      bf16x8 tbf[NP][HEAD_GP_M_MAX / 16];
      float S[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p) S[p] = 0.f;
#pragma unroll
      for (int tt = 0; tt < HEAD_GP_M_MAX / 32; ++tt) {
        if (32 * tt < Mp) {   // (the same for every thread)
#pragma unroll
          for (int q4 = 0; q4 < 4; ++q4) {
            float ca[4] = {0.f, 0.f, 0.f, 0.f};
            for (int o = 0; o < gp.P; ++o) {
              const float wo = aq.wm[o];
              const float4 av = *reinterpret_cast<const float4*>(gp.alpha + (long long)o * Mp + 32 * tt + 8 * q4 + 4 * hh);
              ca[0] = fmaf(wo, av.x, ca[0]);
              ca[1] = fmaf(wo, av.y, ca[1]);
              ca[2] = fmaf(wo, av.z, ca[2]);
              ca[3] = fmaf(wo, av.w, ca[3]);
            }
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
              for (int e = 0; e < 4; ++e)
                kk[tt][p][4 * q4 + e] = fmaf(cB[p], wk[tt][p][4 * q4 + e], cA[p] * ca[e]) * kk[tt][p][4 * q4 + e];
          }
        }
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            uint4 v;
            v.x = pack2bf(kk[tt][p][8 * t], kk[tt][p][8 * t + 1]);
            v.y = pack2bf(kk[tt][p][8 * t + 2], kk[tt][p][8 * t + 3]);
            v.z = pack2bf(kk[tt][p][8 * t + 4], kk[tt][p][8 * t + 5]);
            v.w = pack2bf(kk[tt][p][8 * t + 6], kk[tt][p][8 * t + 7]);
            tbf[p][2 * tt + t] = __builtin_bit_cast(bf16x8, v);
            float f[8];
            unpack8(v, f);
#pragma unroll
            for (int e = 0; e < 8; ++e) S[p] += f[e];
          }
      }
#pragma unroll
      for (int p = 0; p < NP; ++p) S[p] = half_xchg_sum(S[p]);

      // dphi = 2 inv2l2 (tb . zt - phi S) into the registers of h: F output features, K = Mp, the chunk staged at row stride LD0
      const float c2 = 2.f * gp.inv2l2;
      const bf16_t* a = lds + (gc & 1) * BUF + n * LD0 + 8 * hh;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        f32x16 acc[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[p][r] = 0.f;
#pragma unroll
        for (int s = 0; s < HEAD_GP_M_MAX / 16; ++s)
          if (16 * s < Mp) {   // (the same for every thread)
            const bf16x8 af = *reinterpret_cast<const bf16x8*>(a + 32 * mt * LD0 + 16 * s);
#pragma unroll
            for (int p = 0; p < NP; ++p) acc[p] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, tbf[p][s], acc[p], 0, 0, 0);
          }
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            float f[8];
            unpack8(__builtin_bit_cast(uint4, bfr[p][2 * mt + t]), f);
#pragma unroll
            for (int e = 0; e < 8; ++e) h[mt][p][8 * t + e] = c2 * fmaf(-f[e], S[p], acc[p][8 * t + e]);
          }
      }
      stage_store(gc + 1, false);
      __syncthreads();
      ++gc;
    }
  }

  if constexpr (GRAD) {
    // d = cot . wl in the registers of h, the same map
    const float* crow[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) crow[p] = cot + min(row0 + 32 * p + n, N - 1) * ldc;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int r = 0; r < 16; ++r) h[mt][p][r] = 0.f;
    for (int o = 0; o < P; ++o) {
      float c[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p) c[p] = crow[p][o];
      const float* wo = wl + (long long)o * F + 4 * hh;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 wv = *reinterpret_cast<const float4*>(wo + 32 * mt + 8 * q);
#pragma unroll
          for (int p = 0; p < NP; ++p) {
            h[mt][p][4 * q] = fmaf(c[p], wv.x, h[mt][p][4 * q]);
            h[mt][p][4 * q + 1] = fmaf(c[p], wv.y, h[mt][p][4 * q + 1]);
            h[mt][p][4 * q + 2] = fmaf(c[p], wv.z, h[mt][p][4 * q + 2]);
            h[mt][p][4 * q + 3] = fmaf(c[p], wv.w, h[mt][p][4 * q + 3]);
          }
        }
    }
  }

  if constexpr (BACK) {
    // backward layers D - 1 .. 0 (masked operand, d += acc), then rb(d) . w0 as one more layer whose tiles go to memory
    for (int b = 0; b <= D; ++b) {
      const bool lastp = b == D;
      const int l = D - 1 - b;
      bf16x8 bfr[NP][KS];
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const unsigned m = lastp ? 0xffffu : (unsigned)masks[(((long long)l * MT + mt) * NP + p) * NT + tid];
          float dm[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) dm[r] = (m >> r) & 1u ? h[mt][p][r] : 0.f;
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            uint4 v;
            v.x = pack2bf(dm[8 * t], dm[8 * t + 1]);
            v.y = pack2bf(dm[8 * t + 2], dm[8 * t + 3]);
            v.z = pack2bf(dm[8 * t + 4], dm[8 * t + 5]);
            v.w = pack2bf(dm[8 * t + 6], dm[8 * t + 7]);
            bfr[p][2 * mt + t] = __builtin_bit_cast(bf16x8, v);
          }
        }
      if (!lastp) {
#pragma unroll
        for (int i = 0; i < MCH; ++i, ++gc) {
          if (gc + 1 < CT) stage_load(gc + 1, false);
          const bf16_t* a = lds + (gc & 1) * BUF + n * LDR + 8 * hh;
#pragma unroll
          for (int tt = 0; tt < TPC; ++tt) {
            const int mt = i * TPC + tt;
            f32x16 acc[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
              for (int r = 0; r < 16; ++r) acc[p][r] = 0.f;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
              const bf16x8 af = *reinterpret_cast<const bf16x8*>(a + 32 * tt * LDR + 16 * s);
#pragma unroll
              for (int p = 0; p < NP; ++p) acc[p] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr[p][s], acc[p], 0, 0, 0);
            }
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
              for (int r = 0; r < 16; ++r) h[mt][p][r] += acc[p][r];
          }
          if (gc + 1 < CT) stage_store(gc + 1, false);
          __syncthreads();
        }
      } else {
        for (int e0 = 0; e0 < E; e0 += MC, ++gc) {
          if (gc + 1 < CT) stage_load(gc + 1, false);
          const bf16_t* a = lds + (gc & 1) * BUF + n * LDR + 8 * hh;
#pragma unroll
          for (int tt = 0; tt < TPC; ++tt) {
            if (e0 + 32 * tt < E) {   // (the same for every thread)
              f32x16 acc[NP];
#pragma unroll
              for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[p][r] = 0.f;
#pragma unroll
              for (int s = 0; s < KS; ++s) {
                const bf16x8 af = *reinterpret_cast<const bf16x8*>(a + 32 * tt * LDR + 16 * s);
#pragma unroll
                for (int p = 0; p < NP; ++p) acc[p] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr[p][s], acc[p], 0, 0, 0);
              }
#pragma unroll
              for (int p = 0; p < NP; ++p) {
                const long long row = row0 + 32 * p + n;
                if (row < N) {
                  float* gr = g + row * ldg + e0 + 32 * tt + 4 * hh;
#pragma unroll
                  for (int q = 0; q < 4; ++q)
                    *reinterpret_cast<float4*>(gr + 8 * q) = make_float4(acc[p][4 * q], acc[p][4 * q + 1], acc[p][4 * q + 2], acc[p][4 * q + 3]);
                }
              }
            }
          }
          if (gc + 1 < CT) stage_store(gc + 1, false);
          __syncthreads();
        }
      }
    }
  }
}
