// The streaming top-k body of the product-quantised search (pq.hip): topk_stream (topk_stream_dev.h) with ONE change -- where that loads
// 16 bytes of a library row from HBM as the lane's A fragment, this loads one code byte and reads the 16 bytes from the code book in LDS.
// A row of the library is M = E / 8 code bytes; codes[n][m] names the entry of sub-space m (8 bf16 = 16 bytes of cb [M][256][8]) that
// stands for dimensions 8 m .. 8 m + 7.  The A fragment of lane (col, g) at k-step s is A[row = col][k = 32 s + 8 g .. + 7] = dimensions
// 8 (4 s + g) .. + 7 of the row = entry codes[row][4 s + g] of sub-space 4 s + g: one ds_read_b128.
//
// Everything behind the operand is topk_stream's, restated as search8.hip and radius.hip restate it: the k-steps in ascending order from a
// zero accumulator, alpha * acc + bias, the -0 -> +0 step, the strict > against the query's threshold, the appends, the compaction
// (topk_compact) and its barriers.  A (query, row) score therefore has the bits topk_stream gives for the reconstructed bf16 row, and
// every statement of that header about cap, about the barriers being workgroup-uniform and about the written order holds here as it
// stands.
//
// The pipeline is one stage deeper than topk_stream's, because the operand is two dependent reads away: while slab `it` is multiplied,
// the fragments of slab it + 1 are being read from LDS (their code bytes arrived one iteration ago) and the code bytes and bias of slab
// it + 2 are in flight from HBM.  A lane loads the row's code bytes as E / 32 dwords -- dword s holds sub-spaces 4 s .. 4 s + 3, byte g of
// it is the lane's -- so the four lane groups of a row read the same dwords.  A row >= N is read at row N - 1 (inside the allocation)
// and masked by a -inf bias after the MFMA; a slab past the last iteration is never loaded, its registers keep code 0 (entry 0 of the
// sub-space: inside the code book) and its fragments are never multiplied.
//
// START (ivfpq.hip: residual codes inside inverted lists): every slab's accumulator starts from start[p] -- the caller's MFMA chain over
// a part of the row that all rows of the range share, left in all four registers of the lane -- instead of zero, and the k-steps of
// the entries continue that chain.  Without it (pq.hip) every slab starts from zero and `start` is not read.
#pragma once
#include "topk_stream_dev.h"

// Rows [r_begin, r_end) of codes [N, E / 8] (both bounds workgroup-uniform; an empty range leaves empty lists) under the code book cb
// (LDS, [E / 8][256] entries of 16 bytes, complete and behind a barrier when this is called or, as here, behind this function's first
// barrier) against the B fragments bq of panels p < np: topk_stream's arguments and topk_stream's result otherwise.  start [NP]: see START.
template <int KSMAX, int NP, bool START = false>
__device__ __forceinline__ void pq_stream(const unsigned char* __restrict__ codes, long long N, int E, const uint4* cb,
                                          const float* __restrict__ bias, const bf16x8 (&bq)[NP][KSMAX], int np, const bool (&stored)[NP],
                                          long long r_begin, long long r_end, float alpha, int k, int cap, topk_key_t* sbuf, int* s_cnt,
                                          float* s_thr, int* s_flag, const topk_f32x4* start = nullptr) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, g = lane >> 4;
  const int ks = E >> 5, M = E >> 3, nq = 16 * np;
  const int iters = r_end > r_begin ? (int)((r_end - r_begin + TOPK_ROWS_IT - 1) / TOPK_ROWS_IT) : 0;
  if (tid < 16 * NP) {
    s_cnt[tid] = 0;
    s_thr[tid] = -INFINITY;
  }
  if (tid < 2) s_flag[tid] = 0;
  __syncthreads();

  // stage 1, slab -> registers: the row's code dwords and the bias of the lane's four result rows (-inf: masked)
  unsigned c2[KSMAX];
  float b2[4];
#pragma unroll
  for (int s = 0; s < KSMAX; ++s) c2[s] = 0u;
#pragma unroll
  for (int r = 0; r < 4; ++r) b2[r] = -INFINITY;
  auto load_slab = [&](int it) {
    const long long slab = r_begin + 16ll * (4 * it + wave);
    const long long row = min(slab + col, N - 1);
    const unsigned* src = reinterpret_cast<const unsigned*>(codes + row * M);   // (M % 4 == 0: dword aligned)
#pragma unroll
    for (int s = 0; s < KSMAX; ++s)
      if (s < ks) c2[s] = src[s];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long long br = slab + 4 * g + r;
      b2[r] = br < r_end ? (bias ? bias[br] : 0.f) : -INFINITY;
    }
  };
  // stage 2, codes -> fragments: entry (byte g of dword s) of sub-space 4 s + g
  uint4 a1[KSMAX];
  float b1[4];
#pragma unroll
  for (int s = 0; s < KSMAX; ++s) a1[s] = make_uint4(0u, 0u, 0u, 0u);
  auto gather = [&](const unsigned (&c)[KSMAX]) {
#pragma unroll
    for (int s = 0; s < KSMAX; ++s)
      if (s < ks) a1[s] = cb[(4 * s + g) * 256 + ((c[s] >> (8 * g)) & 0xffu)];
  };
  if (iters > 0) {
    load_slab(0);
    gather(c2);
#pragma unroll
    for (int r = 0; r < 4; ++r) b1[r] = b2[r];
    if (iters > 1) load_slab(1);
  }

  for (int it = 0; it < iters; ++it) {
    uint4 ac[KSMAX];
    float bc[4];
#pragma unroll
    for (int s = 0; s < KSMAX; ++s) ac[s] = a1[s];
#pragma unroll
    for (int r = 0; r < 4; ++r) bc[r] = b1[r];
    if (it + 1 < iters) {   // (workgroup-uniform) the codes of slab it + 1 are here: its fragments, then the loads of slab it + 2
      gather(c2);
#pragma unroll
      for (int r = 0; r < 4; ++r) b1[r] = b2[r];
      if (it + 2 < iters) load_slab(it + 2);
    }

    topk_f32x4 acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      if constexpr (START)
        acc[p] = start[p];
      else
        acc[p] = topk_f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int s = 0; s < KSMAX; ++s) {
      if (s < ks) {
#pragma unroll
        for (int p = 0; p < NP; ++p)
          if (p < np) acc[p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ac[s]), bq[p][s], acc[p], 0, 0, 0);
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
          float sc = alpha * acc[p][r] + bc[r];
          sc += 0.0f;   // -0 -> +0: the two must tie
          if (stored[p] && sc > thr) {
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
  }

  topk_compact<true>(sbuf, s_cnt, s_thr, nq, cap, k, wave, lane);
  __syncthreads();
}
