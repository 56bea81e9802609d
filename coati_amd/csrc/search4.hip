// Four-bit library search (include/coati_search4.h): the library as OCP e2m1 nibbles [N, E4 / 2] plus one E8M0 scale byte per 32
// elements [N, E4 / 32] (the OCP Microscaling block format), and a streaming approximate stage over them against e4m3 queries.  The
// exact re-ranking of its candidates is search8.hip's search_rescore_kernel, unchanged.
//
// quant_rows_fp4_kernel, one wave per row, a lane per 8 elements (16 B of bf16 in, 4 B of nibbles out), the 4 lanes of a block reduce
// its largest magnitude: the block exponent j is the smallest integer with amax <= 6 * 2^j = 1.5 * 2^(j + 2) (read from amax's exponent
// and significand, kept in -126 .. 126, 0 for a block of zeros), the element times 2^-j (exact) is rounded to e2m1 by seven compares
// against the midpoints 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5 -- a tie goes to the even code, so > at the midpoints below an even code
// and >= at those below an odd one -- and the sign bit is the product's.  The source is read at its own width E; the lanes between E
// and E4 = 128 ceil(E / 128) write zero nibbles and the scale byte 127.
//
// search4_topk_kernel<T, NP>, grid = (tiles of 16 NP queries) x (S slices), 4 waves -- search8.hip's geometry, its LDS top-k and its
// write-out (topk_key, topk_compact, topk_write_out of topk_stream_dev.h) and its merge (search_merge_kernel).  The stream loop is
// restated here, as search8.hip and radius.hip restate it, with these differences:
//  * the product is v_mfma_scale_f32_16x16x128_f8f6f4 with A = the e4m3 queries (cbsz 0, scale byte 127) and B = the e2m1 rows (blgp 4,
//    the fp4 operand in the first four of its eight registers), T = E4 / 128 of them per slab and panel in ascending order from a zero
//    accumulator.  The QUERIES are the M side here, so the result map (column = lane & 15, row = 4 (lane >> 4) + register) gives a
//    lane the scores of ONE library row (slab + column) against FOUR queries of each panel (4 g + r), and one bias per lane;
//  * operand and scale maps of this form, determined with tools/probes/mx4_probe.hip (profiles/search4_mx_probe.txt): the fp4 operand
//    of lane (c = lane & 15, g = lane >> 4) is 32 consecutive k, 32 g .. 32 g + 31, nibble n of its 16 bytes (low nibble first) = k
//    32 g + n -- ONE scale block, which is the natural load: step t of a row is code bytes 64 t + 16 g .. + 15 -- and the block's scale
//    is read from THAT lane's scale register (byte 0).  The e4m3 operand of lane (i, g) is two runs of 16: registers 0 .. 3 = k 16 g ..
//    16 g + 15, registers 4 .. 7 = k 64 + 16 g .. 64 + 16 g + 15, so a lane's query fragment of step t is the query's bytes
//    128 t + 16 g .. + 15 and 128 t + 64 + 16 g .. + 15.  Nothing is permuted: every element of E4 meets its own scale;
//  * score = (alpha * qscale[q]) * acc + bias[row], then + 0.0f.  alpha and qscale are powers of two, so the factor is exact and so is
//    its product with acc; the rows' scales are applied inside the matrix core;
//  * a slab is a quarter of a bf16 slab's bytes, so the prefetch is deeper again: SEARCH4_NB register buffers, while slab `it` is
//    multiplied the loads of it + 1 .. it + SEARCH4_NB - 1 are in flight, the loop unrolled by SEARCH4_NB so that each step names its
//    buffers statically and no register is copied; no load of the stream is under a condition.  A lane's scale bytes, one per step,
//    are T byte loads (zero-extended: no VALU work).  Measured (profiles/search4_stream_sweep.txt): 3 / 4 / 6 buffers differ by 3 % at
//    most where 6 still fit the registers (at E4 = 512 they do not, and it loses up to 1.9 x), and one packed scale word per step in
//    place of the byte is within 2 % either way: the stream is not what bounds this kernel.  The iteration is still 4 slabs = TOPK_ROWS_IT rows, so the cap arithmetic is
//    topk_stream's unchanged: cap = k + 2 TOPK_ROWS_IT, an iteration appends at most TOPK_ROWS_IT candidates to a query, a compaction
//    runs after every iteration that left a count above cap - TOPK_ROWS_IT and takes every such list to <= k.
// The filter is a strict > against the query's threshold; whether to compact is read by all threads from one LDS word (two, by
// iteration parity) behind a barrier; the trip count comes from blockIdx and the arguments: every barrier is workgroup-uniform.  The
// final compaction orders every list by rank, so what is written does not depend on the order in which the LDS atomics landed.  Rows
// past the slice's end are read at row N - 1 and dropped by the filter.
#include <type_traits>

#include "../../include/coati_search4.h"
#include "search_host.h"

#define SEARCH4_E_MAX 512
#ifndef SEARCH4_NB
#define SEARCH4_NB 4              // register buffers of the stream: SEARCH4_NB - 1 slabs in flight
#endif

typedef int s4_i32x8 __attribute__((ext_vector_type(8)));

// ---- quantiser ---------------------------------------------------------------------------------------------------------------------
// The exponent of a block whose largest magnitude is am (finite): the smallest j with am <= 6 * 2^j = 1.5 * 2^(j + 2), kept in
// -126 .. 126 so that 2^-j is a normal f32 and the scale byte j + 127 is 1 .. 253; 0 for am == 0.
__device__ __forceinline__ int fp4_block_exp(float am) {
  if (am == 0.f) return 0;
  const unsigned u = __float_as_uint(am);
  const int e = (int)((u >> 23) & 0xff) - 127;   // (a subnormal am reads as -127: far below the clamp either way)
  const int j = (u & 0x7fffffu) <= 0x400000u ? e - 2 : e - 1;   // significand <= 1.5 ?
  return max(-126, min(126, j));
}

// the nibble of y, |y| <= 6: sign << 3 | the code of the nearest of {0, 0.5, 1, 1.5, 2, 3, 4, 6}, ties to the even code
__device__ __forceinline__ unsigned fp4_nibble(float y) {
  const float a = fabsf(y);
  const unsigned code = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.0f);
  return code | ((__float_as_uint(y) >> 31) << 3);
}

__global__ __launch_bounds__(256) void quant_rows_fp4_kernel(const bf16_t* __restrict__ x, long long n, int E, int E4,
                                                             unsigned char* __restrict__ codes, unsigned char* __restrict__ scales) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;   // (a whole wave: nothing below crosses waves)
  const bool have = 8 * lane < E;
  float v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = 0.f;
  if (have) {
    const uint4 w = *reinterpret_cast<const uint4*>(x + row * E + 8 * lane);
    const unsigned ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = __uint_as_float(ww[i] << 16);
      v[2 * i + 1] = __uint_as_float(ww[i] & 0xffff0000u);
    }
  }
  float am = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) am = fmaxf(am, fabsf(v[i]));
  am = fmaxf(am, __shfl_xor(am, 1, 64));   // the block's four lanes
  am = fmaxf(am, __shfl_xor(am, 2, 64));
  const int j = fp4_block_exp(am);
  const float inv = __uint_as_float((unsigned)(127 - j) << 23);   // 2^-j
  unsigned word = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) word |= fp4_nibble(v[i] * inv) << (4 * i);
  if (8 * lane < E4) {   // (a lane at or past E holds zeros: nibbles 0, j = 0)
    *reinterpret_cast<unsigned*>(codes + row * (E4 / 2) + 4 * lane) = word;
    if ((lane & 3) == 0) scales[row * (E4 / 32) + (lane >> 2)] = (unsigned char)(j + 127);
  }
}

int coati_quant_rows_fp4(const uint16_t* x, int64_t n, int E, uint8_t* codes, uint8_t* scales, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(x && codes && scales, "quant_rows_fp4: null operand");
  COATI_CHECK_SHAPE(E >= 32 && E <= SEARCH4_E_MAX && E % 32 == 0, "quant_rows_fp4: E=%d is not a multiple of 32 in 32 .. %d", E, SEARCH4_E_MAX);
  COATI_CHECK_SHAPE(n >= 1 && n < (1ll << 31), "quant_rows_fp4: n=%lld outside 1 .. 2^31 - 1", (long long)n);
  const int E4 = (E + 127) / 128 * 128;
  hipLaunchKernelGGL(quant_rows_fp4_kernel, dim3(cdiv(n, 4)), dim3(256), 0, s, x, n, E, E4, codes, scales);
  COATI_LAUNCH_CHECK("quant_rows_fp4");
  return COATI_OK;
}

// ---- stage 1: the stream over the fp4 rows ---------------------------------------------------------------------------------------------
// T: the 128-element steps of a row (E4 = 128 T), NP: the query panels of a workgroup (tiles of 32 queries, as search8.hip's).
template <int T, int NP>
__global__ __launch_bounds__(256) void search4_topk_kernel(const unsigned char* __restrict__ codes, const unsigned char* __restrict__ scales,
                                                           long long N, const float* __restrict__ bias, const unsigned char* __restrict__ q,
                                                           const float* __restrict__ qscale, int Q, int k, float alpha, int S,
                                                           long long slice_rows, int cap, float* __restrict__ part_score,
                                                           int* __restrict__ part_row) {
  extern __shared__ topk_key_t sbuf[];   // [16 NP][cap]
  __shared__ int s_cnt[16 * NP];
  __shared__ float s_thr[16 * NP];
  __shared__ int s_flag[2];
  constexpr int E4 = 128 * T, ROWB = 64 * T, ROWS = 4 * T;   // elements, code bytes and scale bytes of a row
  constexpr int NB = SEARCH4_NB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, g = lane >> 4;
  const int slice = blockIdx.y, q0 = blockIdx.x * 16 * NP;
  const int np = min(NP, (Q - q0 + 15) >> 4), nq = 16 * np;
  const long long r_begin = (long long)slice * slice_rows, r_end = min(N, r_begin + slice_rows);
  const int r_end32 = (int)r_end;   // (< 2^31)
  const int iters = r_end > r_begin ? (int)((r_end - r_begin + TOPK_ROWS_IT - 1) / TOPK_ROWS_IT) : 0;

  // the query tile.  As the A operand lane (col, g) holds query 16 p + col: bytes 128 t + 16 g .. + 15 in registers 0 .. 3, bytes
  // 128 t + 64 + 16 g .. + 15 in registers 4 .. 7 (no query there: zeros).  As the owner of results it has queries 16 p + 4 g + r:
  // qm = alpha * qscale of those, stored = whether there is one
  s4_i32x8 aq[NP][T];
  bool stored[NP][4];
  float qm[NP][4];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int qi = q0 + 16 * p + col;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      uint4 lo = make_uint4(0u, 0u, 0u, 0u), hi = lo;
      if (qi < Q) {
        const unsigned char* src = q + (long long)qi * E4 + 128 * t + 16 * g;
        lo = *reinterpret_cast<const uint4*>(src);
        hi = *reinterpret_cast<const uint4*>(src + 64);
      }
      aq[p][t] = s4_i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qr = q0 + 16 * p + 4 * g + r;
      stored[p][r] = qr < Q;
      qm[p][r] = stored[p][r] ? alpha * qscale[qr] : 0.f;
    }
  }

  if (tid < 16 * NP) {
    s_cnt[tid] = 0;
    s_thr[tid] = -INFINITY;
  }
  if (tid < 2) s_flag[tid] = 0;
  __syncthreads();

  // a wave's slab of iteration it: rows r_begin + 16 (4 it + wave) .. + 15; the lane's row is slab + col, of which it takes block
  // 4 t + g of every step: 16 code bytes, one scale byte; bs = the row's bias.  A row >= N is read at row N - 1 (inside the
  // allocation) and a result row >= r_end is dropped by the filter.  Every load is unconditional -- a load under a lane's or even a
  // uniform condition makes the compiler wait for the slabs in flight where the paths meet
  struct Slab {
    uint4 b[T];
    int sc[T];
    float bs;
  };
  auto load_slab = [&](Slab& d, int it) __attribute__((always_inline)) {
    const long long slab = r_begin + 16ll * (4 * min(it, iters - 1) + wave);   // (past the last iteration: its slab again, never used)
    const long long row = min(slab + col, N - 1);
    const unsigned char* src = codes + row * ROWB + 16 * g;
    const unsigned char* ssrc = scales + row * ROWS + g;
#pragma unroll
    for (int t = 0; t < T; ++t) d.b[t] = *reinterpret_cast<const uint4*>(src + 64 * t);
#pragma unroll
    for (int t = 0; t < T; ++t) d.sc[t] = ssrc[4 * t];
    d.bs = bias[row];
  };
  // one iteration: the slab NB - 1 ahead goes into the buffer the last iteration used, then the products and the filter of `cur`
  auto step = [&](auto refills, int it, const Slab& cur, Slab& refill) __attribute__((always_inline)) {
    if constexpr (decltype(refills)::value) load_slab(refill, it + NB - 1);

    topk_f32x4 acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = topk_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const s4_i32x8 bf = {(int)cur.b[t].x, (int)cur.b[t].y, (int)cur.b[t].z, (int)cur.b[t].w, 0, 0, 0, 0};
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        // (cbsz, blgp) = (0, 4): A e4m3, B e2m1; opsel 0: the scale is byte 0 of the scale register; 127 = 2^0 for the queries
        if (p < np) acc[p] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(aq[p][t], bf, acc[p], 0, 4, 0, 127, 0, cur.sc[t]);
      }
    }

    // filter: the lane's row against the thresholds of its four queries of each panel
    const int row = (int)(r_begin + 16ll * (4 * it + wave)) + col;
    const bool live = row < r_end32;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      if (p < np) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ql = 16 * p + 4 * g + r;
          float sc = qm[p][r] * acc[p][r] + cur.bs;
          sc += 0.0f;   // -0 -> +0: the two must tie
          if (stored[p][r] && live && sc > s_thr[ql]) {
            const int slot = atomicAdd(&s_cnt[ql], 1);   // < cap: the count was <= cap - TOPK_ROWS_IT when this iteration began
            sbuf[ql * cap + slot] = topk_key(sc, row);
            if (slot + 1 > cap - TOPK_ROWS_IT) s_flag[it & 1] = 1;
          }
        }
      }
    }
    __syncthreads();
    const int full = s_flag[it & 1];   // read by every thread between two barriers with no write to it: workgroup-uniform
    if (full) {
      topk_compact<false>(sbuf, s_cnt, s_thr, nq, cap, k, wave, lane);
      __syncthreads();
      if (tid == 0) s_flag[it & 1] = 0;   // (this word's next use is two iterations on, behind the next iteration's barrier)
    }
  };

  Slab buf[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
      buf[j].b[t] = make_uint4(0u, 0u, 0u, 0u);
      buf[j].sc[t] = 127;
    }
    buf[j].bs = 0.f;
  }
  // Whole groups of NB iterations load without any condition -- the counter the compiler waits on must be right on every path, so one
  // path with fewer loads in flight would make all of them wait as if they had as few -- and the up to NB - 1 iterations left over
  // run without loads: what they need is in buf[0 .. NB - 2].  iters, and so every condition here, is workgroup-uniform.
  const int whole = iters / NB * NB;
  if (iters > 0) {
#pragma unroll
    for (int j = 0; j < NB - 1; ++j) load_slab(buf[j], j);
  }
  for (int it = 0; it < whole; it += NB) {
#pragma unroll
    for (int j = 0; j < NB; ++j) step(std::true_type{}, it + j, buf[j], buf[(j + NB - 1) % NB]);
  }
#pragma unroll
  for (int j = 0; j < NB - 1; ++j)
    if (j < iters - whole) step(std::false_type{}, whole + j, buf[j], buf[j]);

  topk_compact<true>(sbuf, s_cnt, s_thr, nq, cap, k, wave, lane);
  __syncthreads();
  topk_write_out(sbuf, s_cnt, cap, k, min(16 * np, Q - q0), ((long long)q0 * S + slice) * k, (long long)S * k, [](int row) { return row; },
                 part_score, part_row);
}

static int search4_check(long long N, int E4, int Q, int k, int S) {
  COATI_TRY(topk_check("search4_topk", N, Q, k, S));
  COATI_CHECK_SHAPE(E4 >= 128 && E4 <= SEARCH4_E_MAX && E4 % 128 == 0, "search4_topk: E4=%d is not a multiple of 128 in 128 .. %d", E4, SEARCH4_E_MAX);
  return COATI_OK;
}

template <int T, int NP>
static int search4_launch(const unsigned char* codes, const unsigned char* scales, long long N, const float* bias, const unsigned char* q,
                          const float* qscale, int Q, int k, float alpha, int S, float* part_score, int* part_row, hipStream_t s) {
  const int cap = k + 2 * TOPK_ROWS_IT;   // <= 256 = 4 candidates per lane of a compacting wave
  // the lists of the panels this launch has: a launch of <= 16 queries takes half the tile's LDS
  const size_t lds = (size_t)16 * min(NP, cdiv(Q, 16)) * cap * sizeof(topk_key_t);
  COATI_TRY((max_dynamic_lds<search4_topk_kernel<T, NP>>("search4_topk", 16 * NP * (TOPK_MAX + 2 * TOPK_ROWS_IT) * (int)sizeof(topk_key_t))));
  hipLaunchKernelGGL((search4_topk_kernel<T, NP>), dim3(cdiv(Q, 16 * NP), S), dim3(256), lds, s, codes, scales, N, bias, q, qscale, Q, k, alpha, S,
                     topk_slice_rows(N, S), cap, part_score, part_row);
  COATI_LAUNCH_CHECK("search4_topk");
  return COATI_OK;
}

int coati_search4_topk(const uint8_t* codes, const uint8_t* scales, int64_t N, int E4, const float* bias, const uint8_t* q,
                       const float* qscale, int Q, int k, float alpha, int S, float* part_score, int32_t* part_row, float* out_score,
                       int64_t* out_row, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(codes && scales && bias && q && qscale && part_score && part_row && out_score && out_row, "search4_topk: null operand");
  COATI_TRY(search4_check(N, E4, Q, k, S));
  switch (E4 / 128) {
    case 1: COATI_TRY((search4_launch<1, 2>(codes, scales, N, bias, q, qscale, Q, k, alpha, S, part_score, part_row, s))); break;
    case 2: COATI_TRY((search4_launch<2, 2>(codes, scales, N, bias, q, qscale, Q, k, alpha, S, part_score, part_row, s))); break;
    case 3: COATI_TRY((search4_launch<3, 2>(codes, scales, N, bias, q, qscale, Q, k, alpha, S, part_score, part_row, s))); break;
    default: COATI_TRY((search4_launch<4, 2>(codes, scales, N, bias, q, qscale, Q, k, alpha, S, part_score, part_row, s))); break;
  }
  return launch_search_merge(part_score, part_row, Q, S * k, k, out_score, LL(out_row), s);
}

// The number of slices coati_search4_topk is given by default: coati_search_slices' (topk_default_slices).  Host arithmetic only.
int coati_search4_slices(int64_t N, int Q, int k) { return topk_default_slices("search4_slices", N, Q, k); }
