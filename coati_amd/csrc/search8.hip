// Quantised library search (include/coati_search8.h): the library as OCP e4m3 bytes [N, E] plus one power-of-two f32 scale per row, a
// streaming approximate stage over them and an exact re-ranking of its candidates from the bf16 rows.
//
// quant_rows_fp8_kernel, one wave per row: the row's largest magnitude by a wave reduction, the scale 2^j with j the smallest integer
// such that amax <= 448 * 2^j (read from amax's exponent and significand, no division, no logarithm), the row times 2^-j (exact) rounded
// to e4m3 by v_cvt_pk_fp8_f32 (round to nearest even; nothing saturates: |x| / s <= 448).
//
// search8_topk_kernel<TMAX, NP>, grid = (tiles of 16 NP queries) x (S slices), 4 waves -- the exact search's geometry (search.hip), its
// LDS top-k and its write-out (topk_key, topk_compact, topk_write_out of topk_stream_dev.h) and its merge (search_merge_kernel).  The
// stream loop is restated here, as radius.hip restates it, with three differences:
//  * the operands are bytes and the product is v_mfma_f32_16x16x32_fp8_fp8 (A, B: 8 bytes per lane, result map as the bf16 form's:
//    column = lane & 15, row = 4 (lane >> 4) + register).  A lane takes 16 CONTIGUOUS bytes of its row per load: load t of lane group g
//    is bytes 64 t + 16 g .. + 15, its low 8 bytes are the fragment of one MFMA and its high 8 bytes of the next.  The queries'
//    fragments are cut the same way, so both operands put the same column of E at the same (MFMA, lane group, byte): the order in
//    which a dot product's terms are summed is a permutation of the natural one and nothing else changes.  E % 64 == 32: the last load
//    exists for g < 2 only: the other lanes hold zeros in the query fragment and any bytes of the row in the other;
//  * score = (alpha * qscale[q] * scale[row]) * acc + bias[row], then + 0.0f.  alpha and the scales are powers of two, so the factor is
//    exact and so is its product with acc;
//  * an fp8 slab is half a bf16 slab's bytes, so the prefetch is one slab deeper: while slab `it` is multiplied, the loads of it + 1
//    and it + 2 are in flight -- 2 x 16 rows x E bytes per wave, what the bf16 kernel keeps in flight with one slab of 2 E bytes a
//    row.  Three register buffers, the loop unrolled by three so that each step names its buffers statically and no register is
//    copied (a copy of a buffer whose load is in flight would wait for it); no load of the stream is under a condition.  The iteration is still 4 slabs = TOPK_ROWS_IT rows, so
//    the cap arithmetic is topk_stream's unchanged: cap = k + 2 TOPK_ROWS_IT, an iteration appends at most TOPK_ROWS_IT candidates to
//    a query, a compaction runs after every iteration that left a count above cap - TOPK_ROWS_IT and takes every such list to <= k:
//    an append never runs past its buffer and no candidate is dropped for lack of room.
// The filter is a strict > against the query's threshold; whether to compact is read by all threads from one LDS word (two, by
// iteration parity) behind a barrier; the trip count comes from blockIdx and the arguments: every barrier is workgroup-uniform.  The
// final compaction orders every list by rank, so what is written does not depend on the order in which the LDS atomics landed.  Rows
// past the slice's end are read at row N - 1 and dropped by the filter.
//
// search_rescore_kernel, one workgroup per query: the <= 128 candidate rows are gathered from the bf16 library as 16-row A slabs (two
// per wave), scored with the exact search's arithmetic -- v_mfma_f32_16x16x32_bf16 over k-steps s = 0 .. E / 32 - 1 from a zero
// accumulator with the query in every B column, alpha * acc + bias, + 0.0f: the bits coati_search_topk gives the pair -- and ranked
// in LDS by topk_compact<true>: score descending, row ascending.
#include <type_traits>

#include "../../include/coati_search8.h"
#include "search_host.h"

#define SEARCH8_E_MAX 512
#define RESCORE_R_MAX 128

// ---- quantiser ---------------------------------------------------------------------------------------------------------------------
// The scale exponent of a row whose largest magnitude is am (finite): the smallest j with am <= 448 * 2^j = 1.75 * 2^(j + 8), kept in
// -126 .. 127 so that 2^j and 2^-j are normal f32; 0 for am == 0.
__device__ __forceinline__ int fp8_scale_exp(float am) {
  if (am == 0.f) return 0;
  const unsigned u = __float_as_uint(am);
  const int e = (int)((u >> 23) & 0xff) - 127;   // (a subnormal am reads as -127: far below the clamp either way)
  const int j = (u & 0x7fffffu) <= 0x600000u ? e - 8 : e - 7;   // significand <= 1.75 ?
  return max(-126, min(127, j));
}

__global__ __launch_bounds__(256) void quant_rows_fp8_kernel(const bf16_t* __restrict__ x, long long n, int E, unsigned char* __restrict__ out,
                                                             float* __restrict__ scale) {
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
#pragma unroll
  for (int d = 1; d < 64; d *= 2) am = fmaxf(am, __shfl_xor(am, d, 64));
  const int j = fp8_scale_exp(am);
  const float inv = __uint_as_float((unsigned)(127 - j) << 23);   // 2^-j
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] *= inv;
  unsigned lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[4], v[5], hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[6], v[7], hi, true);
  if (have) *reinterpret_cast<uint2*>(out + row * E + 8 * lane) = make_uint2(lo, hi);
  if (lane == 0) scale[row] = __uint_as_float((unsigned)(127 + j) << 23);
}

int coati_quant_rows_fp8(const uint16_t* x, int64_t n, int E, uint8_t* out, float* scale, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(x && out && scale, "quant_rows_fp8: null operand");
  COATI_CHECK_SHAPE(E >= 32 && E <= SEARCH8_E_MAX && E % 32 == 0, "quant_rows_fp8: E=%d is not a multiple of 32 in 32 .. %d", E, SEARCH8_E_MAX);
  COATI_CHECK_SHAPE(n >= 1 && n < (1ll << 31), "quant_rows_fp8: n=%lld outside 1 .. 2^31 - 1", (long long)n);
  hipLaunchKernelGGL(quant_rows_fp8_kernel, dim3(cdiv(n, 4)), dim3(256), 0, s, x, n, E, out, scale);
  COATI_LAUNCH_CHECK("quant_rows_fp8");
  return COATI_OK;
}

// ---- stage 1: the stream over the fp8 rows ---------------------------------------------------------------------------------------------
// TMAX: the 16-byte loads of a lane per row (E <= 64 TMAX), NP: the query panels of a workgroup.  Both instantiations take tiles of 32
// queries (NP = 2): at E <= 256 the bf16 kernel's 64-query tile was measured as well and lost in every cell -- its lists of R = 40 and
// more candidates leave room for one workgroup per CU where two of these fit.
template <int TMAX, int NP>
__global__ __launch_bounds__(256) void search8_topk_kernel(const unsigned char* __restrict__ lib, const float* __restrict__ scale, long long N, int E,
                                                           const float* __restrict__ bias, const unsigned char* __restrict__ q,
                                                           const float* __restrict__ qscale, int Q, int k, float alpha, int S,
                                                           long long slice_rows, int cap, float* __restrict__ part_score,
                                                           int* __restrict__ part_row) {
  extern __shared__ topk_key_t sbuf[];   // [16 NP][cap]
  __shared__ int s_cnt[16 * NP];
  __shared__ float s_thr[16 * NP];
  __shared__ int s_flag[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, g = lane >> 4;
  const int slice = blockIdx.y, q0 = blockIdx.x * 16 * NP;
  const int np = min(NP, (Q - q0 + 15) >> 4), nq = 16 * np;
  const long long r_begin = (long long)slice * slice_rows, r_end = min(N, r_begin + slice_rows);
  const int r_end32 = (int)r_end;   // (< 2^31)
  const int iters = r_end > r_begin ? (int)((r_end - r_begin + TOPK_ROWS_IT - 1) / TOPK_ROWS_IT) : 0;

  // which of its loads a lane has: bytes 64 t + 16 g .. + 15 of a row of E bytes (a lane-dependent answer only for the last load of an
  // E that is not a multiple of 64).  A lane without one reads the row's last 16 bytes instead (off: no branch in the stream) against
  // a zero query fragment: the library's bytes are finite e4m3 values, so those products are zeros
  bool has[TMAX];
  int off[TMAX];
#pragma unroll
  for (int t = 0; t < TMAX; ++t) {
    has[t] = 64 * t + 16 * g < E;
    off[t] = min(64 * t + 16 * g, E - 16);
  }

  // the query tile: the same bytes of the query's row; qm = alpha * qscale of the lane's query
  uint4 bq[NP][TMAX];
  bool stored[NP];
  float qm[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int qi = q0 + 16 * p + col;
    stored[p] = qi < Q;
    qm[p] = stored[p] ? alpha * qscale[qi] : 0.f;
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (has[t] && stored[p]) v = *reinterpret_cast<const uint4*>(q + (long long)qi * E + off[t]);
      bq[p][t] = v;
    }
  }

  if (tid < 16 * NP) {
    s_cnt[tid] = 0;
    s_thr[tid] = -INFINITY;
  }
  if (tid < 2) s_flag[tid] = 0;
  __syncthreads();

  // a wave's slab of iteration it: rows r_begin + 16 (4 it + wave) .. + 15; the lane's row is slab + col.  A row >= N is read at row
  // N - 1 (inside the allocation) and a result row >= r_end is dropped by the filter.  bs / ss = the bias and scale of the lane's four
  // result rows.  Every load is unconditional -- a load under a lane's or even a uniform condition makes the compiler wait for the
  // slabs in flight where the paths meet; a lane's load t at or past E (off) repeats the row's last 16 bytes against a zero query fragment
  struct Slab {
    uint4 a[TMAX];
    float bs[4], ss[4];
  };
  auto load_slab = [&](Slab& d, int it) __attribute__((always_inline)) {
    const long long slab = r_begin + 16ll * (4 * min(it, iters - 1) + wave);   // (past the last iteration: its slab again, never used)
    const long long row = min(slab + col, N - 1);
    const unsigned char* src = lib + row * E;
#pragma unroll
    for (int t = 0; t < TMAX; ++t) d.a[t] = *reinterpret_cast<const uint4*>(src + off[t]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long long br = min(slab + 4 * g + r, N - 1);
      d.bs[r] = bias[br];
      d.ss[r] = scale[br];
    }
  };
  // one iteration: the slab two ahead goes into the buffer the last iteration used, then the products and the filter of `cur`
  auto step = [&](auto refills, int it, const Slab& cur, Slab& refill) __attribute__((always_inline)) {
    if constexpr (decltype(refills)::value) load_slab(refill, it + 2);

    topk_f32x4 acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = topk_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
      if (64 * t < E) {
        const long a_lo = (long)(((unsigned long long)cur.a[t].y << 32) | cur.a[t].x);
        const long a_hi = (long)(((unsigned long long)cur.a[t].w << 32) | cur.a[t].z);
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          if (p < np) {
            const long b_lo = (long)(((unsigned long long)bq[p][t].y << 32) | bq[p][t].x);
            const long b_hi = (long)(((unsigned long long)bq[p][t].w << 32) | bq[p][t].z);
            acc[p] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a_lo, b_lo, acc[p], 0, 0, 0);
            acc[p] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a_hi, b_hi, acc[p], 0, 0, 0);
          }
        }
      }
    }

    // filter: the lane's four rows of each panel against its query's threshold
    const int row0 = (int)(r_begin + 16ll * (4 * it + wave)) + 4 * g;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      if (p < np) {
        const int ql = 16 * p + col;
        const float thr = s_thr[ql];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float sc = (qm[p] * cur.ss[r]) * acc[p][r] + cur.bs[r];
          sc += 0.0f;   // -0 -> +0: the two must tie
          if (stored[p] && row0 + r < r_end32 && sc > thr) {
            const int slot = atomicAdd(&s_cnt[ql], 1);   // < cap: the count was <= cap - TOPK_ROWS_IT when this iteration began
            sbuf[ql * cap + slot] = topk_key(sc, row0 + r);
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

  Slab b0, b1, b2;
#pragma unroll
  for (int t = 0; t < TMAX; ++t) b0.a[t] = b1.a[t] = b2.a[t] = make_uint4(0u, 0u, 0u, 0u);
  // Whole triples of iterations load without any condition -- the counter the compiler waits on must be right on every path, so one
  // path with fewer loads in flight would make all of them wait as if they had as few -- and the one or two iterations left over
  // run without loads: what they need is in b0 and b1.  iters, and so every condition here, is workgroup-uniform.
  const int whole = iters / 3 * 3;
  if (iters > 0) {
    load_slab(b0, 0);
    load_slab(b1, 1);
  }
  for (int it = 0; it < whole; it += 3) {
    step(std::true_type{}, it, b0, b2);
    step(std::true_type{}, it + 1, b1, b0);
    step(std::true_type{}, it + 2, b2, b1);
  }
  if (iters - whole >= 1) step(std::false_type{}, whole, b0, b2);
  if (iters - whole == 2) step(std::false_type{}, whole + 1, b1, b0);

  topk_compact<true>(sbuf, s_cnt, s_thr, nq, cap, k, wave, lane);
  __syncthreads();
  topk_write_out(sbuf, s_cnt, cap, k, min(16 * np, Q - q0), ((long long)q0 * S + slice) * k, (long long)S * k, [](int row) { return row; },
                 part_score, part_row);
}

static int search8_check(long long N, int E, int Q, int k, int S) {
  COATI_TRY(topk_check("search8_topk", N, Q, k, S));
  COATI_CHECK_SHAPE(E >= 32 && E <= SEARCH8_E_MAX && E % 32 == 0, "search8_topk: E=%d is not a multiple of 32 in 32 .. %d", E, SEARCH8_E_MAX);
  return COATI_OK;
}

template <int TMAX, int NP>
static int search8_launch(const unsigned char* lib, const float* scale, long long N, int E, const float* bias, const unsigned char* q,
                          const float* qscale, int Q, int k, float alpha, int S, float* part_score, int* part_row, hipStream_t s) {
  const int cap = k + 2 * TOPK_ROWS_IT;   // <= 256 = 4 candidates per lane of a compacting wave
  // the lists of the panels this launch has: a launch of <= 16 queries takes half the tile's LDS
  const size_t lds = (size_t)16 * min(NP, cdiv(Q, 16)) * cap * sizeof(topk_key_t);
  COATI_TRY((max_dynamic_lds<search8_topk_kernel<TMAX, NP>>("search8_topk", 16 * NP * (TOPK_MAX + 2 * TOPK_ROWS_IT) * (int)sizeof(topk_key_t))));
  hipLaunchKernelGGL((search8_topk_kernel<TMAX, NP>), dim3(cdiv(Q, 16 * NP), S), dim3(256), lds, s, lib, scale, N, E, bias, q, qscale, Q, k, alpha,
                     S, topk_slice_rows(N, S), cap, part_score, part_row);
  COATI_LAUNCH_CHECK("search8_topk");
  return COATI_OK;
}

int coati_search8_topk(const uint8_t* lib, const float* scale, int64_t N, int E, const float* bias, const uint8_t* q, const float* qscale,
                       int Q, int k, float alpha, int S, float* part_score, int32_t* part_row, float* out_score, int64_t* out_row,
                       void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(lib && scale && bias && q && qscale && part_score && part_row && out_score && out_row, "search8_topk: null operand");
  COATI_TRY(search8_check(N, E, Q, k, S));
  if (E <= 256)
    COATI_TRY((search8_launch<4, 2>(lib, scale, N, E, bias, q, qscale, Q, k, alpha, S, part_score, part_row, s)));
  else
    COATI_TRY((search8_launch<8, 2>(lib, scale, N, E, bias, q, qscale, Q, k, alpha, S, part_score, part_row, s)));
  return launch_search_merge(part_score, part_row, Q, S * k, k, out_score, LL(out_row), s);
}

// ---- stage 2: the candidates' exact scores ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void search_rescore_kernel(const bf16_t* __restrict__ lib, long long N, int E, const float* __restrict__ bias,
                                                             const bf16_t* __restrict__ q, const long long* __restrict__ cand, int R, int k,
                                                             float alpha, float* __restrict__ out_score, long long* __restrict__ out_row) {
  __shared__ topk_key_t sbuf[RESCORE_R_MAX];
  __shared__ int s_cnt[1];
  __shared__ float s_thr[1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, g = lane >> 4;
  const int ks = E >> 5;
  const long long qi = blockIdx.x;
  if (tid == 0) {
    s_cnt[0] = 0;
    s_thr[0] = -INFINITY;
  }
  __syncthreads();

  // a candidate slot's row, or -1: no candidate there (a pad, a slot >= R, a row outside the library)
  auto cand_row = [&](int slot) -> long long {
    if (slot >= R) return -1;
    const long long c = cand[qi * R + slot];
    return c >= 0 && c < N ? c : -1;
  };
  for (int slab = wave; 16 * slab < R; slab += 4) {   // (R is the workgroup's: no barrier inside anyway)
    // A[row = col][k = 32 s + 8 g + j] of the gathered rows (no candidate: row 0, dropped below), B[k][every column] = the query
    const long long mine = cand_row(16 * slab + col);
    const uint4* src = reinterpret_cast<const uint4*>(lib + max(mine, 0ll) * E + 8 * g);
    const uint4* qsrc = reinterpret_cast<const uint4*>(q + qi * E + 8 * g);
    uint4 a[16], b[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      a[s] = b[s] = make_uint4(0u, 0u, 0u, 0u);
      if (s < ks) {
        a[s] = src[4 * s];
        b[s] = qsrc[4 * s];
      }
    }
    topk_f32x4 acc = topk_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 16; ++s)
      if (s < ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[s]), __builtin_bit_cast(bf16x8, b[s]), acc, 0, 0, 0);
    if (col == 0) {   // every column holds the same query: one lane of each group appends its four rows
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long long row = cand_row(16 * slab + 4 * g + r);
        if (row < 0) continue;
        float sc = alpha * acc[r] + (bias ? bias[row] : 0.f);
        sc += 0.0f;   // -0 -> +0: the two must tie
        if (sc > -INFINITY) sbuf[atomicAdd(&s_cnt[0], 1)] = topk_key(sc, (int)row);   // < R <= 128 appends
      }
    }
  }
  __syncthreads();
  topk_compact<true>(sbuf, s_cnt, s_thr, 1, RESCORE_R_MAX, k, wave, lane);   // rank order: nothing depends on the order of the appends
  __syncthreads();
  if (tid < k) {
    const bool have = tid < s_cnt[0];
    const topk_key_t key = sbuf[tid];
    out_score[qi * k + tid] = have ? topk_key_score(key) : -INFINITY;
    out_row[qi * k + tid] = have ? (long long)topk_key_row(key) : -1;
  }
}

int coati_search_rescore(const uint16_t* lib, int64_t N, int E, const float* bias, const uint16_t* q, int Q, const int64_t* cand, int R, int k,
                         float alpha, float* out_score, int64_t* out_row, void* stream) {
  hipStream_t s = S_(stream);
  COATI_CHECK_ARG(lib && q && cand && out_score && out_row, "search_rescore: null operand");
  COATI_CHECK_SHAPE(E >= 32 && E <= SEARCH8_E_MAX && E % 32 == 0, "search_rescore: E=%d is not a multiple of 32 in 32 .. %d", E, SEARCH8_E_MAX);
  COATI_CHECK_SHAPE(N >= 1 && N < (1ll << 31), "search_rescore: N=%lld outside 1 .. 2^31 - 1", (long long)N);
  COATI_CHECK_SHAPE(Q >= 1, "search_rescore: Q=%d < 1", Q);
  COATI_CHECK_SHAPE(R >= 1 && R <= RESCORE_R_MAX, "search_rescore: R=%d outside 1 .. %d", R, RESCORE_R_MAX);
  COATI_CHECK_SHAPE(k >= 1 && k <= TOPK_MAX, "search_rescore: k=%d outside 1 .. %d", k, TOPK_MAX);
  hipLaunchKernelGGL(search_rescore_kernel, dim3(Q), dim3(256), 0, s, lib, N, E, bias, q, LL(cand), R, k, alpha, out_score, LL(out_row));
  COATI_LAUNCH_CHECK("search_rescore");
  return COATI_OK;
}

// The number of slices coati_search8_topk is given by default: coati_search_slices' (topk_default_slices).  Host arithmetic only.
int coati_search8_slices(int64_t N, int Q, int k) { return topk_default_slices("search8_slices", N, Q, k); }
